"""numpy statements of the two-plane fp16 arithmetic's operand side (csrc/two_plane.hpp: the scale rule;
csrc/lds_async.hpp and csrc/gemm.hip, planes_cut_kernel: the cut and the plane image of include/mmlrec.h,
mml_gemm_planes_cut).  No GPU in here.  tests/test_two_plane_cpu.py holds the C++ header and the C restatement of
oracle/cabi_cpu.c against kexp; the plane-image tests (test_cabi_cpu.py, test_gemm_pipe_gpu.py, test_star_linear_gpu.py)
compare the CPU library and the HIP kernel with planes."""
import numpy as np

AMAX_WORDS = 8  # MML_AMAX_WORDS


def slot(v, word=3):
    """A magnitude slot that holds |v|: the bit pattern in one of its words (producers pick any), zeros elsewhere."""
    s = np.zeros(AMAX_WORDS, dtype=np.uint32)
    s[word] = np.float32(v).view(np.uint32)
    return s


def kexp_bits(bits):
    """The scale exponent of a magnitude bit pattern: k with |x| 2^k < 2^15 (|x| < 2^(e - 126) for the exponent field e),
    Inf / NaN -> 0, clamped to +-110."""
    e = (int(bits) >> 23) & 0xff
    if e == 255:
        return 0
    return int(np.clip(141 - e, -110, 110))


def kexp(v):
    """... of a magnitude given as a number."""
    return kexp_bits(np.float32(v).view(np.uint32))


def cut(W, k):
    """The two-plane cut: h = rne16(w 2^k), l = rne16(w 2^k - h), as uint16 bit patterns (in uint32 arrays)."""
    y = W.astype(np.float32) * np.float32(2.0 ** k)
    h = y.astype(np.float16)
    lo = (y - h.astype(np.float32)).astype(np.float16)
    return h.view(np.uint16).astype(np.uint32), lo.view(np.uint16).astype(np.uint32)


def planes(W, k, layout):
    """The plane image of W cut with exponent k: per block of 16 along the reduction, word 4h + i = h-plane halves
    (S_h[2i], S_h[2i+1]), word 8 + 4h + i = the same of the l plane, S_h = (4h..4h+3, 8+4h..8+4h+3).  layout 0
    (MML_PLANES_ROWS): the reduction runs along a row; 1 (MML_PLANES_COLS): down the rows."""
    hb, lb = cut(W, k)
    if layout == 1:
        hb, lb = hb.T, lb.T  # work on the transpose, transpose back
    out = np.zeros(hb.shape, dtype=np.uint32)
    S = [[4 * h + (e & 3) + 8 * (e >> 2) for e in range(8)] for h in range(2)]
    for b in range(hb.shape[1] // 16):
        blk_h, blk_l = hb[:, 16 * b:16 * b + 16], lb[:, 16 * b:16 * b + 16]
        for h in range(2):
            for i in range(4):
                k0, k1 = S[h][2 * i], S[h][2 * i + 1]
                out[:, 16 * b + 4 * h + i] = blk_h[:, k0] | (blk_h[:, k1] << 16)
                out[:, 16 * b + 8 + 4 * h + i] = blk_l[:, k0] | (blk_l[:, k1] << 16)
    return out.T.copy() if layout == 1 else out
