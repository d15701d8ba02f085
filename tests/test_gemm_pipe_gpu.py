"""Edge cases of the LDS-DMA GEMM kernel (csrc/gemm.hip: gemm_pipe_kernel) against float64 torch: short reductions (the
bias DMA may still be in flight at the epilogue), ragged row / column counts (edge tiles take the drained, uncounted
wait path), outputs that cannot take 16-byte accesses, every activation, multi-problem groups of unequal width,
multi-source + accumulating dgrad, [K,N] weight layout, both tile widths and both arithmetic modes.

Restates nn.Linear + activation (model/utils.py:146-161) and its autograd pair; tolerance = the north star's 1e-4
relative (max-norm), as in tests/test_models_gpu.py.
"""
import os

import numpy as np
import pytest

from two_plane_refs import kexp, planes as planes_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-4


@pytest.fixture(scope="module")
def env():
    import torch
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, ops
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    lib = L.load()
    mode0 = lib.mml_gemm_get_mode()
    lib.mml_gemm_set_ws(0)     # this file pins the TILE kernel (the weight-stationary one: tests/test_gemm_ws_gpu.py)
    yield torch, L, ops, lib
    lib.mml_gemm_set_mode(mode0)
    lib.mml_gemm_set_ws(1)


def rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))


def act_ref(torch, z, act, L):
    if act == L.ACT_RELU:
        return torch.relu(z)
    if act == L.ACT_SIGMOID:
        return torch.sigmoid(z)
    if act == L.ACT_SIGMOID2:
        return 2 * torch.sigmoid(z)
    return z


def dact_ref(torch, y, act, L):
    if act == L.ACT_RELU:
        return (y > 0).double()
    if act == L.ACT_SIGMOID:
        return y * (1 - y)
    if act == L.ACT_SIGMOID2:
        return y * (1 - y / 2)
    return torch.ones_like(y)


@pytest.mark.parametrize("mode", [0, 3, 2])
@pytest.mark.parametrize("M,K,Ns", [
    (128, 16, [64]),            # one k-step per tile
    (300, 32, [128, 4]),        # two k-steps, ragged M, a 4-column problem in the group
    (4096 + 37, 48, [100]),     # three k-steps, N % 64 != 0 (edge tile, 16-byte stores still legal)
    (1000, 240, [256, 256, 64]),
    (260, 64, [130]),           # N % 4 != 0 -> element-wise epilogue
    (70000, 128, [128, 128]),   # > 512 row tiles: persistent workgroups walk several tiles, 128 x 128 tiles
])
def test_pipe_fwd(env, mode, M, K, Ns):
    torch, L, ops, lib = env
    lib.mml_gemm_set_mode(mode)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(M * 7 + K)
    A = torch.randn(M, K, generator=g).to(dev)
    acts = [L.ACT_RELU, L.ACT_NONE, L.ACT_SIGMOID, L.ACT_SIGMOID2]
    probs = []
    for i, N in enumerate(Ns):
        W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
        b = torch.randn(N, generator=g).to(dev) if i % 2 == 0 else None
        probs.append(dict(A=A, W=W, bias=b, C=torch.full((M, N), float("nan"), device=dev), act=acts[i % 4]))
    ops.gemm_fwd(probs, amax=(mode == 2))  # mode 2: two scaled fp16 planes (needs the operand magnitudes)
    if mode == 2:
        assert ", 2, " in lib.mml_gemm_last_kernel().decode()
    torch.cuda.synchronize()
    assert "gemm_pipe_kernel" in lib.mml_gemm_last_kernel().decode()
    for p in probs:
        z = A.double() @ p["W"].double().t()
        if p["bias"] is not None:
            z = z + p["bias"].double()
        assert rel(p["C"], act_ref(torch, z, p["act"], L)) < RTOL


@pytest.mark.parametrize("mode", [0, 3, 2])
@pytest.mark.parametrize("M,K,srcNs,w_kn,act,accumulate", [
    (128, 64, [16], 0, "relu", 0),            # one k-step, Y read in the epilogue
    (515, 256, [128], 0, "relu", 0),          # the layer-2 shape: 8 k-steps + Y
    (515, 240, [256, 256, 64, 64], 0, "none", 0),   # multi-source (layer 1)
    (515, 128, [64, 32], 0, "sigmoid", 1),    # two sources, accumulate into an existing gradient
    (300, 100, [48], 0, "none", 0),           # output width % 64 != 0
    (300, 128, [48, 16], 1, "relu", 0),       # [K,N] weights
    (70000, 128, [128], 0, "relu", 0),
])
def test_pipe_dgrad(env, mode, M, K, srcNs, w_kn, act, accumulate):
    torch, L, ops, lib = env
    lib.mml_gemm_set_mode(mode)
    dev = torch.device("cuda:0")
    act = {"relu": L.ACT_RELU, "none": L.ACT_NONE, "sigmoid": L.ACT_SIGMOID}[act]
    g = torch.Generator(device="cpu").manual_seed(M + K)
    srcs, ref = [], torch.zeros(M, K, dtype=torch.float64, device=dev)
    for N in srcNs:
        dC = torch.randn(M, N, generator=g).to(dev)
        W = (torch.randn(K, N, generator=g) if w_kn else torch.randn(N, K, generator=g)).to(dev) / N ** 0.5
        srcs.append((dC, W, w_kn))
        ref += dC.double() @ (W.double().t() if w_kn else W.double())
    Y = torch.rand(M, K, generator=g).to(dev) - (0.5 if act == L.ACT_RELU else 0.0)
    if act != L.ACT_NONE:
        ref = ref * dact_ref(torch, Y.double(), act, L)
    old = torch.randn(M, K, generator=g).to(dev)
    dA = old.clone() if accumulate else torch.full((M, K), float("nan"), device=dev)
    if accumulate:
        ref = ref + old.double()
    ops.gemm_dgrad([dict(dA=dA, Y=Y if act != L.ACT_NONE else None, act=act, accumulate=accumulate, srcs=srcs)],
                   amax=(mode == 2))
    torch.cuda.synchronize()
    assert "gemm_pipe_kernel" in lib.mml_gemm_last_kernel().decode()
    assert rel(dA, ref) < RTOL


@pytest.mark.parametrize("mode", [0, 3, 2])
@pytest.mark.parametrize("M,shapes,w_kn", [
    (4096, [(64, 16)], 0),
    (4096 + 16, [(256, 240), (64, 240)], 0),     # batch not a multiple of the chunk
    (8192, [(128, 256), (4, 64)], 0),            # a 4-row problem next to a wide one
    (8192, [(100, 48)], 0),                      # N % 64 != 0, K % 64 != 0
    (8192, [(64, 128), (64, 128)], 1),           # [K,N] gradients: bias partials from the column operand
    (70000, [(256, 240)], 0),
])
def test_pipe_wgrad(env, mode, M, shapes, w_kn):
    torch, L, ops, lib = env
    lib.mml_gemm_set_mode(mode)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(M + len(shapes))
    probs, As = [], {}
    for N, K in shapes:
        if K not in As:
            As[K] = torch.randn(M, K, generator=g).to(dev)
        dC = torch.randn(M, N, generator=g).to(dev)
        dW = torch.full((K, N) if w_kn else (N, K), float("nan"), device=dev)
        probs.append(dict(dC=dC, A=As[K], dW=dW, dbias=torch.full((N,), float("nan"), device=dev), w_kn=w_kn))
    ops.gemm_wgrad(probs, amax=(mode == 2))
    torch.cuda.synchronize()
    assert "gemm_pipe_kernel" in lib.mml_gemm_last_kernel().decode()
    for p in probs:
        ref = p["dC"].double().t() @ p["A"].double()
        assert rel(p["dW"], ref.t() if w_kn else ref) < RTOL
        assert rel(p["dbias"], p["dC"].double().sum(0)) < RTOL


def test_pipe_is_bitwise_repeatable(env):
    """Fixed tile order, fixed reduction order: two launches of the same problem give identical bits (the scatter's
    float atomics are the only order-dependent arithmetic of the step)."""
    torch, L, ops, lib = env
    lib.mml_gemm_set_mode(4)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(3)
    M, N, K = 20000, 256, 240
    A, dC = torch.randn(M, K, generator=g).to(dev), torch.randn(M, N, generator=g).to(dev)
    outs = []
    for _ in range(2):
        dW, db = torch.empty(N, K, device=dev), torch.empty(N, device=dev)
        ops.gemm_wgrad([dict(dC=dC, A=A, dW=dW, dbias=db)])
        outs.append((dW.clone(), db.clone()))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("mode", [0, 3, 2])
@pytest.mark.parametrize("M,K,N", [
    (300, 64, 128),      # 128 x 64 tiles (few row tiles): per-lane-row epilogue
    (70000, 128, 256),   # 128 x 128 tiles: row-major epilogue through LDS
    (515, 48, 100),      # ragged columns: last mask word partly used
    (260, 64, 130),      # element-wise epilogue
    (200, 24, 96),       # K % 16 != 0 -> register-staged fallback kernel
])
def test_relu_sign_mask_round_trip(env, mode, M, K, N):
    """Forward writes bit (c & 31) of mask[r, c >> 5] = (relu output > 0); dgrad with the mask == dgrad reading Y."""
    torch, L, ops, lib = env
    lib.mml_gemm_set_mode(mode)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(M + N)
    A = torch.randn(M, K, generator=g).to(dev)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    Cc = torch.empty(M, N, device=dev)
    words = (N + 31) // 32
    mask = torch.full((M, words), -1, dtype=torch.int32, device=dev)
    ops.gemm_fwd([dict(A=A, W=W, bias=b, C=Cc, act=L.ACT_RELU, mask=mask)], amax=(mode == 2))
    torch.cuda.synchronize()
    bits = ((mask.cpu().numpy().astype(np.uint32)[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(M, words * 32)
    assert np.array_equal(bits[:, :N].astype(bool), (Cc > 0).cpu().numpy())
    # next layer's dgrad onto this activation: derivative from the mask vs from Y
    N2 = 64
    dC = torch.randn(M, N2, generator=g).to(dev)
    W2 = (torch.randn(N2, N, generator=g) / N ** 0.5).to(dev)
    d_y, d_m = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
    ops.gemm_dgrad([dict(dA=d_y, Y=Cc, act=L.ACT_RELU, srcs=[(dC, W2, 0)])], amax=(mode == 2))
    ops.gemm_dgrad([dict(dA=d_m, Y=Cc, act=L.ACT_RELU, mask=mask, srcs=[(dC, W2, 0)])], amax=(mode == 2))
    torch.cuda.synchronize()
    assert torch.equal(d_y, d_m)
    ref = (dC.double() @ W2.double()) * (Cc > 0).double()
    assert rel(d_m, ref) < RTOL


@pytest.mark.parametrize("scale_a,scale_w", [(1e-4, 1e-4), (3e-9, 2e3), (5e4, 1e-7), (1.0, 1e-30), (2e20, 1e-20)])
def test_two_plane_fp16_is_scale_invariant(env, scale_a, scale_w):
    """The two-plane fp16 arithmetic (auto mode with operand magnitudes) scales every operand by a power of two taken
    from its magnitude slot: operands far outside fp16's range (the reference initialises weights at 1e-4, gradients
    reach 1e-9) give the same relative accuracy as O(1) ones, and the produced magnitude (amax_out) bounds |C|."""
    torch, L, ops, lib = env
    lib.mml_gemm_set_mode(4)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(11)
    M, K, N = 1000, 240, 256
    A = (torch.randn(M, K, generator=g) * scale_a).to(dev)
    W = (torch.randn(N, K, generator=g) * scale_w).to(dev)
    Cc = torch.empty(M, N, device=dev)
    slots = ops.amax_slots(3, dev)
    ops.amax_batch([(A, slots[0]), (W, slots[1])])
    assert ops.amax_value(slots[0]) == float(A.abs().max()) and ops.amax_value(slots[1]) == float(W.abs().max())
    ops.gemm_fwd([dict(A=A, W=W, bias=None, C=Cc, act=L.ACT_NONE, amax_a=slots[0], amax_w=slots[1], amax_out=slots[2])])
    torch.cuda.synchronize()
    assert ", 2, " in lib.mml_gemm_last_kernel().decode()
    ref = A.double() @ W.double().t()
    assert rel(Cc, ref) < 2e-6
    assert ops.amax_value(slots[2]) == float(Cc.abs().max())
    # a stale-HIGH magnitude (a bound 2^20 above the truth) only costs precision far below the tolerance
    slots[0].fill_(int(np.float32(float(A.abs().max()) * 2.0 ** 20).view(np.int32)))
    ops.gemm_fwd([dict(A=A, W=W, bias=None, C=Cc, act=L.ACT_NONE, amax_a=slots[0], amax_w=slots[1])])
    assert rel(Cc, ref) < 1e-5
    # without magnitudes the same call runs the three-plane bf16 form
    ops.gemm_fwd([dict(A=A, W=W, bias=None, C=Cc, act=L.ACT_NONE)])
    assert ", 3, " in lib.mml_gemm_last_kernel().decode()
    assert rel(Cc, ref) < 2e-6


@pytest.mark.parametrize("ratio", [1e4, 1e8])
def test_two_plane_fp16_with_an_outlier_column_inside_an_operand(env, ratio):
    """The operand scale is per TENSOR (one power of two from the tensor's magnitude), so a wide dynamic range INSIDE one
    operand -- one column `ratio` times larger than the others, e.g. an un-normalised dense feature next to N(0, 1e-4)
    embeddings (reference model/basemodel.py:461-487 concatenates them) -- leaves the small columns low in fp16's range.
    THE CONTRACT IS MAX-NORM: |C - ref| <= 2e-6 max|C| for any operand contents.  Element-wise accuracy of outputs that do
    not see the outlier degrades only once the small entries' low plane goes subnormal, i.e. beyond a ratio of ~2^18
    inside the operand: at 1e4 the outlier-free outputs are still exact to 1e-5 of THEIR OWN magnitude (abs error per
    product <= amax 2^-40 |w|); at 1e8 they keep ~11 bits (the high plane alone) -- stated here, not hidden: a caller with
    such a column normalises it (the reference's dense features are min-max scaled, utils/data_utils.py) or runs
    mml_gemm_set_mode(3).  Forward, input gradient and (tile-kernel) weight gradient, outlier in the A / dC operand."""
    torch, L, ops, lib = env
    lib.mml_gemm_set_mode(4)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(17)
    M, K, N = 1024, 240, 256
    A = torch.randn(M, K, generator=g)
    A[:, 7] *= ratio
    W = torch.randn(N, K, generator=g) / K ** 0.5
    W[N // 2:, 7] = 0.0                      # outputs N/2.. do not see the outlier column
    A, W = A.to(dev), W.to(dev)
    Cc = torch.empty(M, N, device=dev)
    slots = ops.amax_slots(2, dev)
    ops.amax_batch([(A, slots[0]), (W, slots[1])])
    ops.gemm_fwd([dict(A=A, W=W, bias=None, C=Cc, act=L.ACT_NONE, amax_a=slots[0], amax_w=slots[1])])
    torch.cuda.synchronize()
    assert ", 2, " in lib.mml_gemm_last_kernel().decode()
    ref = A.double() @ W.double().t()
    err = (Cc.double() - ref).abs()
    assert float(err.max() / ref.abs().max()) < 2e-6                       # the contract
    own = float(err[:, N // 2:].max() / ref[:, N // 2:].abs().max())       # outlier-free outputs, their own scale
    print("outlier ratio %g: max-norm %.2e, outlier-free block on its own scale %.2e"
          % (ratio, float(err.max() / ref.abs().max()), own))
    assert own < (1e-5 if ratio <= 1e4 else 2e-3)
    # weight gradient dW = dC^T A with the same A (the outlier column of A is the outlier ROW 7 of dW^T): max-norm again,
    # and the outlier-free columns of dW on their own scale
    dC = torch.randn(M, N, generator=g).to(dev)
    dW = torch.empty(N, K, device=dev)
    s2 = ops.amax_slots(1, dev)
    ops.amax_batch([(dC, s2[0])])
    ops.gemm_wgrad([dict(dC=dC, A=A, dW=dW, dbias=None, accumulate=0, amax_dc=s2[0], amax_a=slots[0])])
    torch.cuda.synchronize()
    refw = dC.double().t() @ A.double()
    errw = (dW.double() - refw).abs()
    assert float(errw.max() / refw.abs().max()) < 2e-6
    keep = [k for k in range(K) if k != 7]
    ownw = float(errw[:, keep].max() / refw[:, keep].abs().max())
    assert ownw < (1e-5 if ratio <= 1e4 else 2e-3), ownw
    # input gradient with an outlier column in dC
    dC2 = dC.clone()
    dC2[:, 3] *= ratio
    W2 = (torch.randn(N, K, generator=g) / N ** 0.5).to(dev)
    dA = torch.empty(M, K, device=dev)
    s3 = ops.amax_slots(2, dev)
    ops.amax_batch([(dC2, s3[0]), (W2, s3[1])])
    ops.gemm_dgrad([dict(dA=dA, Y=None, act=L.ACT_NONE, srcs=[(dC2, W2, 0, s3[0], s3[1])])])
    torch.cuda.synchronize()
    refa = dC2.double() @ W2.double()
    assert rel(dA, refa) < 2e-6


def test_amax_of_fallback_kernel_and_nonfinite(env):
    """K % 16 != 0 runs the register-staged fp32 kernel: it must still publish amax_out.  Inf in an operand: scale 1,
    the Inf propagates."""
    torch, L, ops, lib = env
    lib.mml_gemm_set_mode(4)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(5)
    A = torch.randn(200, 24, generator=g).to(dev)
    W = torch.randn(96, 24, generator=g).to(dev)
    Cc = torch.empty(200, 96, device=dev)
    slots = ops.amax_slots(3, dev)
    ops.amax_batch([(A, slots[0]), (W, slots[1])])
    ops.gemm_fwd([dict(A=A, W=W, bias=None, C=Cc, act=L.ACT_RELU, amax_a=slots[0], amax_w=slots[1], amax_out=slots[2])])
    assert "gemm_kernel" in lib.mml_gemm_last_kernel().decode()
    assert ops.amax_value(slots[2]) == float(Cc.abs().max())
    A2 = torch.randn(256, 64, generator=g).to(dev)
    A2[3, 5] = float("inf")
    W2 = torch.randn(64, 64, generator=g).to(dev)
    C2 = torch.empty(256, 64, device=dev)
    s2 = ops.amax_slots(2, dev)
    ops.amax_batch([(A2, s2[0]), (W2, s2[1])])
    ops.gemm_fwd([dict(A=A2, W=W2, bias=None, C=C2, act=L.ACT_NONE, amax_a=s2[0], amax_w=s2[1])])
    assert not torch.isfinite(C2[3]).all() and torch.isfinite(C2[4]).all()


@pytest.mark.parametrize("scale_w", [1e-4, 1.0, 3e5])
def test_planes_cut_image_and_exponent(env, scale_w):
    """mml_gemm_planes_cut against the numpy restatement: both layouts, a pitched weight, a group of two magnitudes."""
    torch, L, ops, lib = env
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(5)
    N, K = 96, 80
    buf = torch.zeros(N, K + 16, device=dev)
    W = buf[:, :K]
    W.copy_((torch.randn(N, K, generator=g) * scale_w).to(dev))
    W2 = (torch.randn(48, 64, generator=g) * scale_w * 8).to(dev)
    slots = ops.amax_slots(2, dev)
    ops.amax_batch([(W, slots[0]), (W2, slots[1])])
    pr = torch.zeros(N, K + 16, dtype=torch.int32, device=dev)[:, :K]
    pc = torch.zeros(N, K + 16, dtype=torch.int32, device=dev)[:, :K]
    p2 = torch.zeros(48, 64, dtype=torch.int32, device=dev)
    kx = torch.full((3,), 12345, dtype=torch.int32, device=dev)
    ops.planes_cut([(W, pr, ops.PLANES_ROWS, [slots[0]], kx[0:1]),
                    (W, pc, ops.PLANES_COLS, [slots[0], slots[1]], kx[1:2]),   # group of two: the larger magnitude rules
                    (W2, p2, ops.PLANES_COLS, [slots[1], slots[0]], kx[2:3])])
    torch.cuda.synchronize()
    k_own = kexp(float(W.abs().max()))
    k_grp = min(k_own, kexp(float(W2.abs().max())))
    assert kx.tolist() == [k_own, k_grp, k_grp]
    Wn = W.cpu().numpy()
    assert np.array_equal(pr.cpu().numpy().view(np.uint32), planes_ref(Wn, k_own, 0))
    assert np.array_equal(pc.cpu().numpy().view(np.uint32), planes_ref(Wn, k_grp, 1))
    assert np.array_equal(p2.cpu().numpy().view(np.uint32), planes_ref(W2.cpu().numpy(), k_grp, 1))
    with pytest.raises(L.MMLError):  # reduction extent not a multiple of 16 and no room for the rounded-up block
        ops.planes_cut([(W[:, :72], torch.zeros(N, 72, dtype=torch.int32, device=dev), ops.PLANES_ROWS, [slots[0]], kx[0:1])])
    with pytest.raises(L.MMLError):  # reduction down the rows: the row count must be a multiple of 16
        ops.planes_cut([(W[:40], pc[:40], ops.PLANES_COLS, [slots[0]], kx[0:1])])
    # the zero-padded operand of a ragged reduction (K = 72 -> 80): planes of the padded shape cut from the weight itself
    Wr = W[:, :72]
    pp = torch.zeros(N, 80, dtype=torch.int32, device=dev)
    pq = torch.full((N, 80), 0, dtype=torch.int32, device=dev)
    ops.planes_cut([(Wr, pp, ops.PLANES_ROWS, [slots[0]], kx[0:1]), (Wr, pq, ops.PLANES_COLS, [slots[0]], kx[1:2])])
    torch.cuda.synchronize()
    Wpad = np.zeros((N, 80), dtype=np.float32)
    Wpad[:, :72] = Wr.cpu().numpy()
    assert np.array_equal(pp.cpu().numpy().view(np.uint32), planes_ref(Wpad, k_own, 0))
    assert np.array_equal(pq.cpu().numpy().view(np.uint32), planes_ref(Wpad, k_own, 1))


@pytest.mark.parametrize("M,K,Ns", [(1000, 240, [256, 256, 64]), (70000, 128, [128, 128]), (300, 32, [128, 4]),
                                    (4096 + 37, 48, [100])])
def test_pipe_fwd_with_precut_weights_is_bitwise_the_in_kernel_cut(env, M, K, Ns, monkeypatch):
    """Forward launches whose weights arrive as pre-cut planes give the SAME bits as the launches that cut the weight
    fragments in registers (same planes, same products, same order), and run the planes kernel."""
    torch, L, ops, lib = env
    lib.mml_gemm_set_mode(4)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(M + K)
    A = (torch.randn(M, K, generator=g) * 3e-3).to(dev)
    Ws = [(torch.randn(n, K, generator=g) * 1e-4).to(dev) for n in Ns]
    bs = [torch.randn(n, generator=g).to(dev) * 1e-6 for n in Ns]
    slots = ops.amax_slots(1 + len(Ns), dev)
    ops.amax_batch([(A, slots[0])] + [(w, slots[1 + i]) for i, w in enumerate(Ws)])
    planes = [torch.zeros(w.shape, dtype=torch.int32, device=dev) for w in Ws]
    kx = torch.zeros(len(Ns), dtype=torch.int32, device=dev)
    ops.planes_cut([(w, p, ops.PLANES_ROWS, [slots[1 + i]], kx[i:i + 1]) for i, (w, p) in enumerate(zip(Ws, planes))])
    outs = []
    for use in (False, True):
        Cs = [torch.empty(M, n, device=dev) for n in Ns]
        probs = [dict(A=A, W=w, bias=b, C=c, act=L.ACT_RELU, amax_a=slots[0], amax_w=slots[1 + i])
                 for i, (w, b, c) in enumerate(zip(Ws, bs, Cs))]
        if use:
            for i, p in enumerate(probs):
                p.update(w_planes=planes[i], w_kexp=kx[i:i + 1])
        ops.gemm_fwd(probs)
        torch.cuda.synchronize()
        name = lib.mml_gemm_last_kernel().decode()
        assert ", 2, false" in name and name.endswith(", true>") == use, name
        outs.append([c.cpu().numpy() for c in Cs])
    for a, b, w, bias in zip(outs[0], outs[1], Ws, bs):
        assert np.array_equal(a, b)
        ref = torch.relu(A.double() @ w.double().t() + bias.double())
        assert rel(torch.from_numpy(b).to(dev), ref) < 2e-6


def test_pipe_fwd_dgrad_with_precut_padded_weights(env):
    """Ragged reduction (K = 72, the operands zero-padded to 80 as engine.LinearGroupOp does): planes of the padded shape,
    cut from the unpadded weight, give the bits of the launches that read the padded float copy."""
    torch, L, ops, lib = env
    lib.mml_gemm_set_mode(4)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(3)
    M, K, KP, N = 3000, 72, 80, 128
    Ap = torch.zeros(M, KP, device=dev)
    Ap[:, :K] = (torch.randn(M, K, generator=g) * 2e-3).to(dev)
    W = (torch.randn(N, K, generator=g) * 1e-4).to(dev)
    Wp = torch.zeros(N, KP, device=dev)
    Wp[:, :K] = W
    dC = (torch.randn(M, N, generator=g) * 1e-6).to(dev)
    slots = ops.amax_slots(3, dev)
    ops.amax_batch([(Ap, slots[0]), (W, slots[1]), (dC, slots[2])])
    pr = torch.zeros(N, KP, dtype=torch.int32, device=dev)
    pc = torch.zeros(N, KP, dtype=torch.int32, device=dev)
    kx = torch.zeros(2, dtype=torch.int32, device=dev)
    ops.planes_cut([(W, pr, ops.PLANES_ROWS, [slots[1]], kx[0:1]), (W, pc, ops.PLANES_COLS, [slots[1]], kx[1:2])])
    outs = []
    for use in (False, True):
        Cc = torch.empty(M, N, device=dev)
        p = dict(A=Ap, W=Wp, bias=None, C=Cc, act=L.ACT_NONE, amax_a=slots[0], amax_w=slots[1])
        if use:
            p.update(w_planes=pr, w_kexp=kx[0:1])
        ops.gemm_fwd([p])
        torch.cuda.synchronize()
        assert lib.mml_gemm_last_kernel().decode().endswith(", true>") == use
        dA = torch.zeros(M, KP, device=dev)
        ops.gemm_dgrad([dict(dA=dA, Y=None, act=L.ACT_NONE, accumulate=0,
                             srcs=[(dC, Wp, 0, slots[2], slots[1]) + ((pc, kx[1:2]) if use else ())])])
        torch.cuda.synchronize()
        assert lib.mml_gemm_last_kernel().decode().endswith(", true>") == use
        outs.append((Cc.cpu().numpy(), dA.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert rel(torch.from_numpy(outs[1][0]).to(dev), Ap.double() @ Wp.double().t()) < 2e-6
    assert float(np.abs(outs[1][1][:, K:]).max()) == 0.0  # the padding columns of the input gradient stay zero


@pytest.mark.parametrize("M,K,srcNs,accumulate", [(1000, 240, [256, 256, 64, 64], 0), (70000, 256, [128], 1),
                                                  (300, 64, [48, 16], 0)])
def test_pipe_dgrad_with_precut_weights_is_bitwise_the_in_kernel_cut(env, M, K, srcNs, accumulate):
    """The same for the input gradient: the weights of a problem's sources are cut as ONE group (common exponent)."""
    torch, L, ops, lib = env
    lib.mml_gemm_set_mode(4)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(M + K + 1)
    dCs = [(torch.randn(M, n, generator=g) * 1e-6).to(dev) for n in srcNs]
    Ws = [(torch.randn(n, K, generator=g) * (1e-4 * (1 + 3 * i))).to(dev) for i, n in enumerate(srcNs)]
    ns = len(srcNs)
    slots = ops.amax_slots(2 * ns, dev)
    ops.amax_batch([(t, slots[i]) for i, t in enumerate(dCs + Ws)])
    planes = [torch.zeros(w.shape, dtype=torch.int32, device=dev) for w in Ws]
    kx = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.planes_cut([(w, p, ops.PLANES_COLS, [slots[ns + i] for i in range(ns)], kx) for w, p in zip(Ws, planes)])
    base = torch.randn(M, K, generator=g).to(dev) * 1e-9
    outs = []
    for use in (False, True):
        dA = base.clone()
        srcs = [(dCs[i], Ws[i], 0, slots[i], slots[ns + i]) + ((planes[i], kx) if use else ()) for i in range(ns)]
        ops.gemm_dgrad([dict(dA=dA, Y=None, act=L.ACT_NONE, accumulate=accumulate, srcs=srcs)])
        torch.cuda.synchronize()
        name = lib.mml_gemm_last_kernel().decode()
        assert ", 2, false" in name and name.endswith(", true>") == use, name
        outs.append(dA.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    ref = sum(dc.double() @ w.double() for dc, w in zip(dCs, Ws)) + (base.double() if accumulate else 0)
    assert rel(torch.from_numpy(outs[1]).to(dev), ref) < 2e-6
