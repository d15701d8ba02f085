"""The deterministic scatter's two opt-in forms (include/mmlrec.h, mml_scatter_bwd_det flags): the magnitude of dOut
supplied by the caller instead of measured by the call, and the row totals left in the 64-bit accumulators for
mml_opt_step_dense (mml_opt_tensor.acc64) instead of a launch that moves them into the fp32 gradient tables.  Neither
changes a bit of the step: path A (the default call, then the marked dense update) against path B (both flags, then
the dense update that converts the totals itself)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VOCAB = [2, 100, 1000, 5000, 300000]   # a hot two-row table, direct-mapped, hashed and large tables
B = 5000                               # ten chunks of 512 samples (more than the 8 XCD slots), ragged last chunk
ZERO_ROW = 77                          # row of table 2 that only receives +x and -x: marked, total exactly zero


@pytest.fixture(scope="module")
def env():
    import torch
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, ops
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch, L, ops


def _batches(torch, E, nonfinite):
    """Two steps' (X, d): gradients over eight decades (as the stand-alone kernel test draws them)."""
    F = len(VOCAB)
    g = torch.Generator().manual_seed(100 + E)
    out = []
    for step in range(2):
        X = torch.stack([(torch.rand(B, generator=g) ** 3 * v).floor().clamp_(0, v - 1) for v in VOCAB], 1).contiguous()
        d = torch.randn(B, F * E, generator=g) * torch.logspace(-6, 2, B).unsqueeze(1)[torch.randperm(B, generator=g)]
        # the zero-total row: nobody else may hit it, two samples carry x and -x
        X[X[:, 2] == ZERO_ROW, 2] = ZERO_ROW + 1
        X[10, 2] = X[4001, 2] = ZERO_ROW
        d[4001, 2 * E:3 * E] = -d[10, 2 * E:3 * E]
        if nonfinite:
            d[3210, 4 * E + 2] = float("nan")
        if nonfinite == "inf_nan":
            d[123, 3 * E + 1] = float("inf")
        out.append((X, d.contiguous()))
    return out


def _run_path(torch, L, ops, E, kind, l2, cap, fused, batches, nonfinite):
    dev = torch.device("cuda:0")
    F = len(VOCAB)
    # mml_opt_step_dense honours marks in its streaming launch only (>= 2^24 parameters): a ballast table with no marked
    # row (its own all-zero map, no totals) rides along in the optimizer launch and is compared too
    shapes = VOCAB + [(1 << 24) // E + 3]
    g = torch.Generator().manual_seed(7)
    small = [torch.randn(v, E, generator=g) for v in VOCAB]
    gd = torch.Generator(device=dev).manual_seed(8)
    tabs = [t.to(dev) for t in small] + [torch.randn(shapes[-1], E, generator=gd, device=dev)]
    s1 = [torch.rand(v, E, generator=gd, device=dev) for v in shapes]
    s2 = [torch.rand(v, E, generator=gd, device=dev) for v in shapes]
    grads = [torch.zeros(v, E, device=dev) for v in shapes]
    acc = [torch.zeros(v, E, dtype=torch.int64, device=dev) for v in VOCAB]
    marks = torch.zeros(ops.marks_bytes(VOCAB), dtype=torch.uint8, device=dev)
    ballast_marks = torch.zeros(shapes[-1], dtype=torch.uint8, device=dev)
    base = np.concatenate([[0], np.cumsum([(v + 31) // 32 * 32 for v in VOCAB])]).tolist()
    mk = [marks[base[f]:base[f] + VOCAB[f]] for f in range(F)] + [ballast_marks]
    slot = ops.amax_slots(1, dev)[0]
    shift = ops.scatter_det_shift(B)
    reg = (0.0, l2) if l2 else None
    for step, (X, d) in enumerate(batches, 1):
        Xd, dd = X.to(dev), d.to(dev)
        if fused:
            slot.zero_()
            ops.amax_batch([(dd, slot)])
            ops.scatter_bwd_det(grads[:F], Xd, list(range(F)), dd, acc, marks, amax_slot=slot, clear_marks=False,
                                amax_supplied=True, defer_totals=True)
            assert int(mk[2][ZERO_ROW]) == 1 and int(acc[2][ZERO_ROW].abs().max()) == 0
            # (an Inf in dOut is the launch's magnitude: every finite addend is below the fixed-point unit, all totals 0)
            assert any(int(a.abs().max()) > 0 for a in acc) or nonfinite == "inf_nan"
        else:
            ops.scatter_bwd_det(grads[:F], Xd, list(range(F)), dd, acc, marks, amax_slot=slot, clear_marks=False)
        hyper = ops.make_hyper(kind, 0.01, step=step, zero_grad=True, max_blocks=cap)
        ents = []
        for f in range(F + 1):
            det = (acc[f], slot, shift) if (fused and f < F) else None
            ents.append((tabs[f], grads[f], s1[f] if kind != "sgd" else None, s2[f] if kind == "adam" else None,
                         reg, None, mk[f], det))
        ops.opt_step_dense(ents, hyper)
        torch.cuda.synchronize()
        if fused:
            assert all(int(a.abs().max()) == 0 for a in acc), step
            assert int(marks.max()) == 0 and int(ballast_marks.max()) == 0, step
            for f in range(F):
                gz = grads[f].view(torch.int32) & 0x7fffffff
                assert int(gz.max()) == 0, (step, f)
    return tabs, s1, s2


def _bits_equal(torch, a, b, nan_aware):
    ai, bi = a.view(torch.int32), b.view(torch.int32)
    if not nan_aware:
        return torch.equal(ai, bi)
    both_nan = torch.isnan(a) & torch.isnan(b)
    return bool(((ai == bi) | both_nan).all())


def _twin(env, E, nonfinite):
    torch, L, ops = env
    batches = _batches(torch, E, nonfinite)
    # Adam and SGD, then Adam with l2 on the tables; the capped grid (U chunks in flight per thread) and the full one
    for kind, l2, cap in (("adam", 0.0, 300), ("sgd", 0.0, 0), ("adam", 1e-3, 1 << 20)):
        a = _run_path(torch, L, ops, E, kind, l2, cap, False, batches, nonfinite)
        b = _run_path(torch, L, ops, E, kind, l2, cap, True, batches, nonfinite)
        for which, (ta, tb) in enumerate(zip(a, b)):
            if (which == 1 and kind == "sgd") or (which == 2 and kind != "adam"):
                continue  # (state the optimizer does not have)
            for f in range(len(ta)):
                assert _bits_equal(torch, ta[f], tb[f], bool(nonfinite)), (kind, l2, cap, which, f)
        del a, b


@pytest.mark.parametrize("E", [4, 8, 16])
def test_deferred_totals_and_supplied_magnitude_give_the_default_paths_bits(env, E):
    """(a) two consecutive steps per path: parameters and both moments bit-equal; on the fused path the 64-bit totals,
    the marks and the fp32 gradient tables are all zero after every step (asserted inside the path)."""
    _twin(env, E, nonfinite=None)


@pytest.mark.parametrize("what", ["inf_nan", "nan"])
@pytest.mark.parametrize("E", [4, 8, 16])
def test_nonfinite_addends_reach_the_update_the_same_way(env, E, what):
    """(b) one Inf and one NaN in dOut: the fold kernel adds them to the fp32 table directly, the optimizer's
    grad + from_fixed(total) sees them like the finalize launch's dst += from_fixed(total) did.  The NaN alone (it never
    registers in the magnitude) leaves the finite addends their totals: a row then holds a NaN in `grad` AND totals."""
    _twin(env, E, nonfinite=what)


def test_acc64_needs_marks_and_excludes_skip_rows(env):
    """(c) argument errors, raised by the host function before any launch."""
    torch, L, ops = env
    dev = torch.device("cuda:0")
    E, V = 8, (1 << 24) // 8
    p = torch.ones(V, E, device=dev)
    z = [torch.ones_like(p) for _ in range(3)]
    acc = torch.zeros(V, E, dtype=torch.int64, device=dev)
    slot = ops.amax_slots(1, dev)[0]
    marks = torch.zeros(V, dtype=torch.uint8, device=dev)
    skip = torch.zeros((V + 31) // 32, dtype=torch.int32, device=dev)
    hyper = ops.make_hyper("adam", 0.01, step=1)
    det = (acc, slot, ops.scatter_det_shift(4096))
    lib = L.load()
    for ent in ((p, z[0], z[1], z[2], None, None, None, det),      # no marks
                (p, z[0], z[1], z[2], None, skip, marks, det),     # skip_rows beside the marks
                (p, z[0], z[1], z[2], None, None, marks, (acc.view(-1)[1:], slot, det[2]))):   # misaligned totals
        arr = ops.make_opt_tensors([ent])
        rc = lib.mml_opt_step_dense(arr, 1, ctypes.byref(hyper), None)
        assert rc == L.ERR_ARG, rc
        assert b"acc64" in lib.mml_last_error()
    torch.cuda.synchronize()
    assert float(p.min()) == 1.0 and float(p.max()) == 1.0   # nothing ran (a step from g = 1 would have moved p)


@pytest.mark.parametrize("M", [16384, 16384 + 77])
def test_dgrad_magnitude_slot_is_the_exact_maximum_of_what_it_stored(env, M):
    """(d) the smallest launch csrc/gemm_os.hip serves (M = 16 384 rows, K = 192 columns, two sources, 256 reduction
    columns in all) and one whose row count is not a multiple of its panel: the slot raised through amax_out holds, bit
    for bit, the largest word mml_amax_batch measures over the stored gradient -- what lets the deterministic scatter
    take its fixed-point unit from the producer."""
    torch, L, ops = env
    dev = torch.device("cuda:0")
    lib = L.load()
    mode0 = lib.mml_gemm_get_mode()
    lib.mml_gemm_set_mode(4)
    try:
        K, Ns = 192, [128, 128]
        g = torch.Generator().manual_seed(M)
        slots = ops.amax_slots(2 * len(Ns) + 2, dev)
        kexp = torch.zeros(1, dtype=torch.int32, device=dev)
        srcs, wslots = [], []
        for s, N in enumerate(Ns):
            dC = (torch.randn(M, N, generator=g) * (1.0 + s)).to(dev)
            W = (torch.randn(N, K, generator=g) / sum(Ns) ** 0.5).to(dev)
            sd, sw = slots[2 * s], slots[2 * s + 1]
            ops.amax_batch([(dC, sd), (W, sw)])
            wslots.append(sw)
            srcs.append([dC, W, 0, sd, sw, torch.zeros((N, K), dtype=torch.int32, device=dev), kexp])
        ops.planes_cut([(s[1], s[5], ops.PLANES_COLS, wslots, kexp) for s in srcs])
        dA = torch.full((M, K), float("nan"), device=dev)
        out_slot, ref_slot = slots[-2], slots[-1]
        ops.gemm_dgrad([dict(Y=None, act=L.ACT_NONE, mask=None, amax_out=out_slot, srcs=[tuple(s) for s in srcs],
                             dA=dA, accumulate=0)])
        torch.cuda.synchronize()
        assert lib.mml_gemm_last_kernel().decode() == "gemm_os_kernel"
        ops.amax_batch([(dA, ref_slot)])
        torch.cuda.synchronize()
        got, want = int(out_slot.view(torch.int32).max()), int(ref_slot.view(torch.int32).max())
        assert got == want and got == int(dA.abs().max().view(torch.int32)), (got, want)
    finally:
        lib.mml_gemm_set_mode(mode0)
