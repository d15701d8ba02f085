"""The scale rule of the two-plane fp16 arithmetic (csrc/two_plane.hpp) off the GPU.  tests/two_plane_driver.cpp, a
stand-alone program around the header's pure part, is compiled with g++; it prints the scale exponent of a sweep of bit
patterns, held here against the numpy statement (tests/two_plane_refs.py), and checks the rule's properties itself (the
exponent's range, 2^k, the two clauses that keep kA + kB inside fp32's range).  The C restatement of oracle/cabi_cpu.c
(amax_exp, kept independent on purpose) goes through the same sweep, so the header, numpy and C are held to each other."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

from conftest import ROOT
from two_plane_refs import AMAX_WORDS, kexp_bits

# all 256 exponent fields x mantissa all-zeros / all-ones x sign clear / set
SWEEP = [sign | (e << 23) | mant for e in range(256) for mant in (0, 0x7fffff) for sign in (0, 0x80000000)]
PROPERTIES = ["pow2_bits", "scale_exp_range", "row_gives_way", "both_give_way"]
_tmp = None


@functools.lru_cache(maxsize=None)
def driver_lines():
    """The output of the compiled driver (built and run once per session)."""
    global _tmp
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import build
    _tmp = tempfile.TemporaryDirectory()
    exe = os.path.join(_tmp.name, "two_plane_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", build.CSRC,
                           os.path.join(ROOT, "tests", "two_plane_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout.splitlines()


def test_scale_exponent_is_the_numpy_statement():
    got = {int(w[1], 16): int(w[2]) for w in (ln.split() for ln in driver_lines()) if w[0] == "exp"}
    assert sorted(got) == sorted(SWEEP)
    assert got == {b: kexp_bits(b) for b in SWEEP}
    # (the numpy statement itself at a few values worked out by hand: 1.0 -> 2^14, 65504 -> 2^-1 x, Inf, 0, the clamps)
    assert [kexp_bits(b) for b in (0x3f800000, 0x477fe000, 0x7f800000, 0x7fc00000, 0, 0x0f000000, 0x0f800000,
                                   0x7d800000, 0x7e000000)] == [14, -1, 0, 0, 110, 110, 110, -110, -110]


def test_rule_properties_hold():
    lines = driver_lines()
    assert not [ln for ln in lines if ln.startswith("FAIL")]
    assert [ln.split()[1] for ln in lines if ln.startswith("ok")] == PROPERTIES


def test_cpu_library_exponent_is_the_same_rule():
    """mml_gemm_planes_cut of the CPU library (oracle/cabi_cpu.c: amax_exp) writes the exponent of a one-slot group: the
    same sweep, one matrix per bit pattern."""
    from oracle import build_fast
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L
    lib = C.CDLL(build_fast.build_cabi())
    lib.mml_gemm_planes_cut.restype, lib.mml_gemm_planes_cut.argtypes = L._SIGS["mml_gemm_planes_cut"]
    n = len(SWEEP)
    W = np.zeros((1, 16), dtype=np.float32)
    out = np.zeros((n, 16), dtype=np.uint32)
    kx = np.full(n, 12345, dtype=np.int32)
    slots = np.zeros((n, AMAX_WORDS), dtype=np.uint32)
    slots[np.arange(n), np.arange(n) % AMAX_WORDS] = SWEEP  # (any word of the slot)
    arr = (L.PlanesDesc * n)()
    for i in range(n):
        d = arr[i]
        d.W, d.planes, d.rows, d.ld, d.cols, d.layout, d.n_amax = W.ctypes.data, out[i].ctypes.data, 1, 16, 16, 0, 1
        d.amax[0] = slots[i].ctypes.data
        d.kexp = kx[i:i + 1].ctypes.data
    assert lib.mml_gemm_planes_cut(arr, n, None) == 0
    assert kx.tolist() == [kexp_bits(b) for b in SWEEP]
