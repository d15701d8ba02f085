"""mml_scatter_pool_bwd_det in isolation: the deterministic form of the pooled scatter (include/mmlrec.h, next to K2p).

Grid: E in {4, 8, 16} x maxlen in {1, 5, 64, 256} x B in {1, 64, 1000}, Zipf ids, all six (combiner, mode) pairs at
once, in the case layout of tests/test_pooled_rows_gpu.py (a 50-row table: the direct-mapped path; a 5 000-row table
shared by a single-valued and a pooled field: the hashed path and shared totals; three dense columns).  maxlen 1 and 5
are a lane-group size and a non power of two, 256 leaves one sample per workgroup at E = 16, B = 1000 a ragged last
workgroup and rows that receive addends from many workgroups.

Per case: (1) two calls on fresh buffers give the same bits; (2) so does the batch with its rows permuted; (3) every
element lies within  n * u / 2 + 2^-24 * sum |addend| + 2^-24 * |ref64|  of the float64 sum -- n addends each rounded
once to the unit u = 2^(emax - 150 - shift), the one fp32 division of a mean block, the final conversion; emax from
d_out on the host, shift from the rule; nothing here is taken from what the kernel gives -- and rows no valid position
names are bitwise 0; (4) the totals are zero after a call that finalizes, the marks cleared on request and otherwise
set exactly on the valid rows per table; (5) a magnitude slot filled beforehand gives the same bits; (6) deferred
totals leave the fp32 gradient alone and from_fixed of them, on the host, is the gradient of (1) bit for bit.
Then: a NaN addend reaches its fp32 row and disturbs nothing else, an out-of-range id at a valid position sets the
status word and adds nothing, and the refusals launch nothing.  And a schema of single-valued fields alone leaves the
same totals and marks as mml_scatter_bwd_det, bit for bit: the two kernels share one fold (csrc/scatter_fold.hpp)."""
import itertools

import numpy as np
import pytest
import torch

from test_pooled_rows_gpu import PAIRS, Case

pytestmark = pytest.mark.gpu

ES, TS, BS = (4, 8, 16), (1, 5, 64, 256), (1, 64, 1000)


def device_inputs(case, dev):
    from mmlrec_amd import ops
    tabs = [torch.from_numpy(t).to(dev) for t in case.tables]
    X = torch.from_numpy(case.X).to(dev)
    _, argmax, _ = ops.gather_pool_fwd(tabs, X, case.singles, case.fields(), case.dense_col0, case.nd)
    return X, torch.from_numpy(case.d_out).to(dev), argmax


def scatter(case, dev, X, d_out, argmax, grad_fill=0.0, **kw):
    """One call on fresh buffers -> (gradients, totals, marks, status) as numpy."""
    from mmlrec_amd import ops
    grads = [torch.full((v, case.E), grad_fill, dtype=torch.float32, device=dev) for v in case.vocab]
    acc = [torch.zeros((v, case.E), dtype=torch.int64, device=dev) for v in case.vocab]
    marks = torch.zeros(ops.marks_bytes(case.vocab), dtype=torch.uint8, device=dev)
    status = ops.new_status(dev)
    ops.scatter_pool_bwd_det(grads, X, case.singles, case.fields(), d_out, acc, marks, argmax=argmax, status=status, **kw)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in grads], [a.cpu().numpy() for a in acc], marks.cpu().numpy(), int(status.item())


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def reference(case, arg_dev):
    """Per table, float64 [V, E]: the sum of the addends, their number and the sum of their magnitudes.  arg_dev: the
    argmax bytes the backward follows (uint8 [B, P * E])."""
    E, B = case.E, case.B
    G = [np.zeros((v, E)) for v in case.vocab]
    N = [np.zeros((v, E)) for v in case.vocab]
    S = [np.zeros((v, E)) for v in case.vocab]
    d = case.d_out.astype(np.float64)

    def add(tb, rows, w, counted=None):
        V = case.vocab[tb]
        for e in range(E):
            G[tb][:, e] += np.bincount(rows, weights=w[:, e], minlength=V)
            S[tb][:, e] += np.bincount(rows, weights=np.abs(w[:, e]), minlength=V)
            N[tb][:, e] += np.bincount(rows if counted is None else rows[counted[:, e]], minlength=V)

    for f, (c, tb) in enumerate(case.singles):
        add(tb, case.X[:, c].astype(np.int64), d[:, f * E:(f + 1) * E])
    for p, (c0, T, comb, tb, lc) in enumerate(case.pooled):
        ids, valid = case.ids[p], case.valid[p]
        blk = d[:, (2 + p) * E:(3 + p) * E]
        bi, ti = np.nonzero(valid)
        rows = ids[bi, ti]
        if comb == "max":  # dOut[e] where argmax[e] == t, 0 (an exact addend: not counted) elsewhere
            sel = arg_dev[:, p * E:(p + 1) * E].astype(np.int64)[bi] == ti[:, None]
            add(tb, rows, np.where(sel, blk[bi], 0.0), counted=sel)
            continue
        if comb == "mean":  # (float)n + 1e-8f, then the quotient: the kernel's one fp32 division is the 2^-24 term
            n = valid.sum(1)
            blk = blk / (n.astype(np.float32) + np.float32(1e-8)).astype(np.float64)[:, None]
        add(tb, rows, blk[bi])
    return G, N, S


def check_marks(case, m, want):
    base = 0
    for t, v in enumerate(case.vocab):
        assert np.array_equal(np.nonzero(m[base:base + v])[0], want[t]), f"marks of table {t}"
        assert not m[base + v:base + 32 * ((v + 31) // 32)].any()
        base += 32 * ((v + 31) // 32)


@pytest.mark.parametrize("E,T,B", list(itertools.product(ES, TS, BS)), ids=lambda v: str(v))
def test_deterministic_pooled_scatter(E, T, B):
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import ops
    dev = torch.device("cuda:0")
    case = Case(E, T, B, "zipf", tuple(PAIRS), seed=E * 100003 + T * 1009 + B)
    X, d_out, argmax = device_inputs(case, dev)
    want_rows = case.valid_rows()
    shift = ops.scatter_pool_det_shift((case.vocab, E, case.singles, case.fields()), B)
    assert 4 <= shift <= 28
    # ---- (1) repeatable, (4) totals consumed and marks cleared
    g1, acc1, m1, st1 = scatter(case, dev, X, d_out, argmax)
    g2, _, _, _ = scatter(case, dev, X, d_out, argmax)
    assert st1 == 0
    assert same_bits(g1, g2)
    assert not any(a.any() for a in acc1) and not m1.any()
    # ---- (2) independent of the order of the samples
    perm = torch.from_numpy(np.random.default_rng(B + T).permutation(B)).to(dev)
    g3, _, _, _ = scatter(case, dev, X[perm].contiguous(), d_out[perm].contiguous(), argmax[perm].contiguous())
    assert same_bits(g1, g3)
    # ---- (3) accuracy against float64, bound derived from the number formats
    amax = np.abs(case.d_out).max()
    emax = int(np.clip((np.float32(amax).view(np.uint32) >> 23) & 0xff, 1, 254))
    u = 2.0 ** (emax - 150 - shift)
    G, N, S = reference(case, argmax.cpu().numpy())
    for t in range(len(case.vocab)):
        err = np.abs(g1[t].astype(np.float64) - G[t])
        bound = N[t] * u / 2 + 2.0 ** -24 * S[t] + 2.0 ** -24 * np.abs(G[t])
        print(f"[pooled det] E={E} T={T} B={B} table {t}: shift={shift} max err/bound = "
              f"{float((err / np.maximum(bound, 1e-300)).max()):.3g}, most addends on an element {int(N[t].max())}")
        assert np.all(err <= bound), (t, float((err - bound).max()))
        idle = np.ones(case.vocab[t], bool)
        idle[want_rows[t]] = False
        assert not g1[t][idle].view(np.uint32).any(), "a row no valid position names must stay bitwise 0"
    # ---- (4) without CLEAR_MARKS: exactly the valid rows of every table stay marked
    g4, acc4, m4, _ = scatter(case, dev, X, d_out, argmax, clear_marks=False)
    assert same_bits(g1, g4) and not any(a.any() for a in acc4)
    check_marks(case, m4, want_rows)
    # ---- (5) the magnitude supplied by the caller
    slot = ops.amax_slots(1, dev)[0]
    slot.zero_()
    ops.amax_batch([(d_out, slot)])
    g5, acc5, m5, _ = scatter(case, dev, X, d_out, argmax, amax_slot=slot, amax_supplied=True)
    assert same_bits(g1, g5) and not any(a.any() for a in acc5) and not m5.any()
    # ---- (6) deferred totals: the fp32 gradient is not written, the totals are the gradient
    g6, acc6, m6, _ = scatter(case, dev, X, d_out, argmax, grad_fill=1.5, clear_marks=False, defer_totals=True)
    assert all(np.array_equal(g.view(np.uint32), np.full_like(g, 1.5).view(np.uint32)) for g in g6)
    check_marks(case, m6, want_rows)
    host = [np.ldexp(a.astype(np.float64), emax - 150 - shift).astype(np.float32) for a in acc6]
    assert same_bits(g1, host)


@pytest.mark.parametrize("E", ES)
def test_single_valued_and_pooled_kernels_are_one_fold(E):
    """scatter_fold_kernel and scatter_pool_fold_kernel share one insert and one flush (csrc/scatter_fold.hpp): a
    schema of single-valued fields alone -- tables of 3 (hot, direct-mapped), 50 (direct-mapped) and 5 000 rows (hashed)
    -- sent through both deterministic scatters with the same magnitude slot and deferred totals leaves the same
    64-bit totals, bit for bit (exact integer sums of the same to_fixed values: no tolerance), and the same marks.
    B = 1000: a ragged last chunk at both chunk sizes (512 lookups at E = 4 and 8, 256 at E = 16)."""
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import ops
    from test_pooled_rows_gpu import draw_ids
    dev = torch.device("cuda:0")
    B, vocab = 1000, (3, 50, 5000)
    rng = np.random.default_rng(4242 + E)
    Xh = np.stack([draw_ids(rng, "zipf", v, B, 0) for v in vocab], axis=1).astype(np.float32)
    g = torch.Generator().manual_seed(E)
    d = torch.randn(B, 3 * E, generator=g) * torch.logspace(-6, 2, B).unsqueeze(1)[torch.randperm(B, generator=g)]
    X, d_out = torch.from_numpy(Xh).to(dev), d.to(dev)
    singles = [(f, f) for f in range(3)]
    # the two shift rules agree at this B (mml_scatter_det_shift, mml_scatter_pool_det_shift)
    assert ops.scatter_det_shift(B) == 28
    assert ops.scatter_pool_det_shift((vocab, E, singles, []), B) == 28
    slot = ops.amax_slots(1, dev)[0]
    ops.amax_batch([(d_out, slot)])

    def run(pooled_kernel):
        grads = [torch.zeros(v, E, device=dev) for v in vocab]
        acc = [torch.zeros(v, E, dtype=torch.int64, device=dev) for v in vocab]
        marks = torch.zeros(ops.marks_bytes(vocab), dtype=torch.uint8, device=dev)
        status = ops.new_status(dev)
        kw = dict(amax_slot=slot, clear_marks=False, status=status, amax_supplied=True, defer_totals=True)
        if pooled_kernel:
            ops.scatter_pool_bwd_det(grads, X, singles, [], d_out, acc, marks, **kw)
        else:
            ops.scatter_bwd_det(grads, X, [0, 1, 2], d_out, acc, marks, **kw)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        return [x.cpu().numpy() for x in grads], [a.cpu().numpy() for a in acc], marks.cpu().numpy()

    g_s, acc_s, m_s = run(False)
    g_p, acc_p, m_p = run(True)
    assert any(a.any() for a in acc_s)
    for t in range(3):
        assert np.array_equal(acc_s[t], acc_p[t]), f"totals of table {t}"
        assert not g_s[t].view(np.uint32).any() and not g_p[t].view(np.uint32).any()
    assert np.array_equal(m_s, m_p)
    base = 0
    for t, v in enumerate(vocab):  # (and they are the rows of the batch)
        assert np.array_equal(np.nonzero(m_s[base:base + v])[0], np.unique(Xh[:, t].astype(np.int64)))
        base += 32 * ((v + 31) // 32)


def test_nan_addend_reaches_its_row_and_nothing_else_moves():
    import mmlrec_amd  # noqa: F401
    dev = torch.device("cuda:0")
    case = Case(8, 5, 64, "zipf", tuple(PAIRS), seed=5)
    X, d_out, argmax = device_inputs(case, dev)
    d_out[3, 2] = 0.0  # (single-valued field 0, element 2)
    clean, _, _, _ = scatter(case, dev, X, d_out, argmax)
    d_out[3, 2] = float("nan")  # a NaN does not register in the magnitude: the unit stays what it was
    got, acc, _, _ = scatter(case, dev, X, d_out, argmax)
    row = int(case.X[3, 0])
    assert np.isnan(got[0][row, 2]) and not any(a.any() for a in acc)
    got[0][row, 2] = clean[0][row, 2]
    assert same_bits(clean, got)


def test_status_at_a_valid_position_adds_nothing():
    """An out-of-range id at a valid position sets `status` and adds nothing: with dOut = 1 the one row every other
    position names holds the count of those positions, exactly (1.0 is a whole number of units)."""
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import ops
    dev = torch.device("cuda:0")
    E, T, B, V = 8, 6, 32, 100
    X = np.zeros((B, T + 1), np.float32)
    X[:, :3] = 5
    X[:, T] = 3
    X[7, 1] = V + 50
    Xd = torch.from_numpy(X).to(dev)
    pf = [ops.PooledField(0, T, "sum", 0, T)]
    g = [torch.zeros(V, E, device=dev)]
    acc = [torch.zeros(V, E, dtype=torch.int64, device=dev)]
    marks = torch.zeros(ops.marks_bytes([V]), dtype=torch.uint8, device=dev)
    status = ops.new_status(dev)
    ops.scatter_pool_bwd_det(g, Xd, [], pf, torch.ones(B, E, device=dev), acc, marks, status=status, clear_marks=False)
    assert int(status.item()) == 2
    want = np.zeros((V, E), np.float32)
    want[5] = 3 * B - 1
    assert np.array_equal(g[0].cpu().numpy(), want)
    assert np.nonzero(marks.cpu().numpy())[0].tolist() == [5]


def test_refusals_return_err_arg_and_launch_nothing():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, ops
    dev = torch.device("cuda:0")
    case = Case(8, 5, 64, "zipf", tuple(PAIRS), seed=11)
    X, d_out, argmax = device_inputs(case, dev)
    grads = [torch.zeros(v, 8, device=dev) for v in case.vocab]
    acc = [torch.zeros(v, 8, dtype=torch.int64, device=dev) for v in case.vocab]
    marks = torch.zeros(ops.marks_bytes(case.vocab), dtype=torch.uint8, device=dev)
    slot = ops.amax_slots(1, dev)[0]
    slot.fill_(0x12345)  # (a call that got as far as its magnitude pass would reset it)
    for kw in (dict(acc64=acc, flags=L.SCATTER_DET_DEFER_TOTALS | L.SCATTER_DET_CLEAR_MARKS),
               dict(acc64=None, flags=0),
               dict(acc64=acc, flags=8),
               dict(acc64=acc, flags=L.SCATTER_DET_CLEAR_MARKS | 64)):
        with pytest.raises(L.MMLError) as ei:
            ops.scatter_pool_bwd_det(grads, X, case.singles, case.fields(), d_out, kw["acc64"], marks, argmax=argmax,
                                     amax_slot=slot, flags=kw["flags"])
        assert f"code {L.ERR_ARG}" in str(ei.value), str(ei.value)
    torch.cuda.synchronize()
    assert not any(bool(g.view(torch.int32).any()) for g in grads) and not any(bool(a.any()) for a in acc)
    assert not bool(marks.any()) and bool((slot.view(torch.int32) == 0x12345).all())
