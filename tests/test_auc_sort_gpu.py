"""mml_auc_sorted (csrc/auc_sort.hip): AUC of segments of any length, with masks, on the MI355X.

Two references.  (1) An integer restatement in numpy: sort the participating negatives, searchsorted left / right for every
positive; the kernel's (2U, P, N) must equal it EXACTLY.  (2) sklearn.metrics.roc_auc_score on the float64 image of the
same fp32 scores, within the tolerance tests/test_kernels_gpu.py uses for mml_auc_segments against sklearn (1e-12)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SKLEARN_TOL = 1e-12  # tests/test_kernels_gpu.py::test_auc_segments_match_sklearn
NONFINITE = 16       # bit 4 of the status word


def dev():
    return torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@pytest.fixture(scope="module")
def ops():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import ops as o
    return o


@pytest.fixture(scope="module")
def tile(ops):
    from mmlrec_amd import _lib as L
    t = int(L.load().mml_auc_sorted_tile())
    assert t >= 256
    return t


SCORE_SETS = ("distinct", "quantised", "equal", "ascending", "descending", "zero_one", "denormal", "signed_zero", "signed")


def scores(kind, n, rng):
    if kind == "distinct":
        return ((rng.permutation(n) + 1.0) / (n + 1.0)).astype(np.float32)
    if kind == "quantised":  # 8 values: heavy ties
        return (np.round(rng.random(n) * 7) / 7).astype(np.float32)
    if kind == "equal":
        return np.full(n, 0.5, np.float32)
    if kind == "ascending":
        return np.sort(rng.random(n).astype(np.float32))
    if kind == "descending":
        return np.sort(rng.random(n).astype(np.float32))[::-1].copy()
    if kind == "zero_one":
        return rng.choice(np.array([0.0, 1.0, 0.5], np.float32), n)
    if kind == "denormal":  # bit patterns 0 .. 39 with either sign: +-0 and the smallest denormals
        bits = rng.integers(0, 40, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)
        return bits.view(np.float32)
    if kind == "signed_zero":
        return rng.choice(np.array([-0.0, 0.0, 1e-3, -1e-3], np.float32), n)
    if kind == "signed":
        return (rng.standard_normal(n) * 5).astype(np.float32)
    raise KeyError(kind)


def ref_counts(p, lab):
    """(2U, P, N) of fp32 scores p and boolean labels lab, in integers."""
    s = p.astype(np.float64)
    neg = np.sort(s[~lab])
    pos = s[lab]
    two_u = int(np.searchsorted(neg, pos, "left").astype(np.int64).sum() +
                np.searchsorted(neg, pos, "right").astype(np.int64).sum())
    return two_u, int(lab.sum()), int((~lab).sum())


def run(ops, pred, y, seg=0, mask=None):
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    auc, counts = ops.auc_sorted(pred, y, seg=seg, mask=mask, return_counts=True, status=status)
    return auc.cpu().numpy(), counts.cpu().numpy(), int(status.item())


def check(pred, y, got_auc, got_counts, seg=0, mask=None, sklearn=True):
    """pred / y (/ mask) host arrays [n, cols]; compares every (segment, column) problem with both references."""
    from sklearn.metrics import roc_auc_score
    n, cols = pred.shape
    seg = n if seg <= 0 or seg >= n else seg
    nseg = (n + seg - 1) // seg
    assert got_auc.shape == (nseg, cols) and got_counts.shape == (nseg, cols, 3)
    for s in range(nseg):
        sl = slice(s * seg, min(n, (s + 1) * seg))
        for c in range(cols):
            p, lab = pred[sl, c], y[sl, c] > 0.5
            if mask is not None:
                m = mask[sl, c if mask.shape[1] > 1 else 0] != 0
                p, lab = p[m], lab[m]
            want = ref_counts(p, lab)
            assert tuple(int(v) for v in got_counts[s, c]) == want, (s, c, got_counts[s, c], want)
            if want[1] == 0 or want[2] == 0:
                assert np.isnan(got_auc[s, c]), (s, c)
                continue
            assert got_auc[s, c] == want[0] / (2.0 * want[1] * want[2])
            if sklearn:
                ref = roc_auc_score(lab, p.astype(np.float64))
                assert abs(got_auc[s, c] - ref) < SKLEARN_TOL, (s, c, got_auc[s, c], ref)


def all_sets(n, seed):
    rng = np.random.default_rng(seed)
    pred = np.stack([scores(k, n, rng) for k in SCORE_SETS], 1)
    y = (rng.random(pred.shape) < 0.4).astype(np.float32)
    return pred, y


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 70001])
def test_score_sets_small_and_16bit_ranks(ops, n):
    """Every score set as one column; 70 001 rows: more than 65 536 keys per problem (16-bit ranks would wrap)."""
    pred, y = all_sets(n, n)
    auc, counts, status = run(ops, T(pred), T(y))
    assert status == 0
    check(pred, y, auc, counts)


@pytest.mark.parametrize("where", ["tile-1", "tile", "tile+1", "3tiles+5"])
def test_score_sets_around_the_scatter_tile(ops, tile, where):
    n = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "3tiles+5": 3 * tile + 5}[where]
    pred, y = all_sets(n, n)
    auc, counts, status = run(ops, T(pred), T(y))
    assert status == 0
    check(pred, y, auc, counts)


def test_million_rows_64bit_pair_counts(ops):
    """(1 << 20) + 3 rows, balanced classes: P * N is about 2.7e11, far beyond 32 bits."""
    n = (1 << 20) + 3
    rng = np.random.default_rng(7)
    pred = np.stack([rng.random(n).astype(np.float32), (np.round(rng.random(n) * 7) / 7).astype(np.float32)], 1)
    y = (rng.random((n, 2)) < 0.5).astype(np.float32)
    auc, counts, status = run(ops, T(pred), T(y))
    assert status == 0
    assert int(counts[0, 0, 1]) * int(counts[0, 0, 2]) > 1 << 37
    check(pred, y, auc, counts)


def test_block_of_several_tiles(ops, tile):
    """A workgroup takes more than one tile once a problem is longer than 512 tiles (its running digit offsets carry
    from tile to tile): 512 tiles + one more + 5 rows, the last block ragged.  Integer reference only (sklearn adds
    nothing the million-row case does not cover)."""
    n = 513 * tile + 5
    rng = np.random.default_rng(11)
    pred = (rng.standard_normal((n, 1)) * 3).astype(np.float32)
    pred[::5] = np.round(pred[::5])  # ties among distinct values
    y = (rng.random((n, 1)) < 0.3).astype(np.float32)
    auc, counts, status = run(ops, T(pred), T(y))
    assert status == 0
    check(pred, y, auc, counts, sklearn=False)


def test_columns_with_padded_rows(ops):
    """cols = 3 inside wider matrices: ldp > cols and ldy > cols."""
    n = 3001
    rng = np.random.default_rng(3)
    big_p = rng.standard_normal((n, 5)).astype(np.float32)
    big_y = (rng.random((n, 7)) < 0.4).astype(np.float32)
    tp, ty = T(big_p)[:, :3], T(big_y)[:, :3]
    assert tp.stride(0) == 5 and ty.stride(0) == 7
    auc, counts, status = run(ops, tp, ty)
    assert status == 0
    check(big_p[:, :3], big_y[:, :3], auc, counts)


def test_segments_ragged_tail(ops):
    n, seg = 12345, 5000
    pred, y = all_sets(n, 5)
    auc, counts, status = run(ops, T(pred), T(y), seg=seg)
    assert status == 0 and auc.shape[0] == 3
    check(pred, y, auc, counts, seg=seg)


def test_segments_of_4096_equal_auc_segments(ops):
    """Same integers either way: at seg = 4096 the doubles of the one-workgroup kernel are reproduced bit for bit."""
    n, seg = 12345, 4096
    rng = np.random.default_rng(9)
    pred = np.stack([rng.random(n).astype(np.float32), scores("quantised", n, rng), scores("signed_zero", n, rng)], 1)
    y = (rng.random((n, 3)) < 0.3).astype(np.float32)
    y[:seg, 2] = 1.0  # one single-class problem: NaN in both
    auc, counts, _ = run(ops, T(pred), T(y), seg=seg)
    old = ops.auc_segments(T(pred), T(y), seg).cpu().numpy()
    assert np.isnan(old[0, 2]) and np.isnan(auc[0, 2])
    assert np.array_equal(np.isnan(auc), np.isnan(old))
    assert np.array_equal(np.nan_to_num(auc, nan=-1.0), np.nan_to_num(old, nan=-1.0))  # equal doubles
    check(pred, y, auc, counts, seg=seg)


def test_masks(ops):
    n, seg = 9001, 4000
    rng = np.random.default_rng(13)
    pred = np.stack([rng.random(n).astype(np.float32), scores("quantised", n, rng), scores("signed", n, rng)], 1)
    y = (rng.random((n, 3)) < 0.4).astype(np.float32)
    shared = (rng.random((n, 1)) < 0.5).astype(np.float32)
    per_col = (rng.random((n, 3)) < 0.5).astype(np.float32) * 3.0  # any non-zero value takes the row in
    for seg_ in (0, seg):
        plain = run(ops, T(pred), T(y), seg=seg_)
        check(pred, y, plain[0], plain[1], seg=seg_)
        for m in (shared, per_col):
            auc, counts, status = run(ops, T(pred), T(y), seg=seg_, mask=T(m))
            assert status == 0
            check(pred, y, auc, counts, seg=seg_, mask=m)
    auc, counts, status = run(ops, T(pred), T(y), mask=T(np.zeros((n, 1), np.float32)))
    assert status == 0 and np.isnan(auc).all() and not counts.any()
    # a random half == the unmasked call on the compacted rows, integers included
    keep = shared[:, 0] != 0
    auc_m, counts_m, _ = run(ops, T(pred), T(y), mask=T(shared))
    auc_c, counts_c, _ = run(ops, T(pred[keep]), T(y[keep]))
    assert np.array_equal(counts_m, counts_c) and np.array_equal(auc_m, auc_c)


def test_single_class_is_nan(ops):
    n = 5000
    rng = np.random.default_rng(2)
    pred = rng.random((n, 2)).astype(np.float32)
    y = np.stack([np.ones(n, np.float32), np.zeros(n, np.float32)], 1)
    auc, counts, status = run(ops, T(pred), T(y))
    assert status == 0 and np.isnan(auc).all()
    assert counts[0, 0].tolist() == [0, n, 0] and counts[0, 1].tolist() == [0, 0, n]


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_score(ops, bad):
    n, seg = 6000, 2500
    rng = np.random.default_rng(4)
    pred = rng.standard_normal((n, 2)).astype(np.float32)
    y = (rng.random((n, 2)) < 0.4).astype(np.float32)
    mask = np.ones((n, 1), np.float32)
    mask[3000] = 0.0
    clean = run(ops, T(pred), T(y), seg=seg, mask=T(mask))
    assert clean[2] == 0
    dirty = pred.copy()
    dirty[3000, 1] = bad  # at a masked-out row: nothing changes
    got = run(ops, T(dirty), T(y), seg=seg, mask=T(mask))
    assert got[2] == 0 and np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1])
    dirty = pred.copy()
    dirty[3001, 1] = bad  # at a participating row of problem (segment 1, column 1)
    auc, counts, status = run(ops, T(dirty), T(y), seg=seg, mask=T(mask))
    assert status & NONFINITE
    assert np.isnan(auc[1, 1])
    others = np.ones_like(auc, bool)
    others[1, 1] = False
    assert np.array_equal(auc[others], clean[0][others]) and np.array_equal(counts[others], clean[1][others])


def test_repeatable_and_order_independent(ops):
    n, seg = 20011, 7000
    pred, y = all_sets(n, 21)
    first = run(ops, T(pred), T(y), seg=seg)
    again = run(ops, T(pred), T(y), seg=seg)
    assert np.array_equal(first[1], again[1]) and np.array_equal(first[0].view(np.int64), again[0].view(np.int64))
    rng = np.random.default_rng(22)
    perm = np.concatenate([s + rng.permutation(min(seg, n - s)) for s in range(0, n, seg)])
    shuffled = run(ops, T(pred[perm]), T(y[perm]), seg=seg)
    assert np.array_equal(first[1], shuffled[1]) and np.array_equal(first[0].view(np.int64), shuffled[0].view(np.int64))


def test_graph_capture_replays_on_changed_inputs(ops):
    n, seg = 10007, 4500
    sets = [all_sets(n, 30 + i) for i in range(3)]
    m0 = (np.random.default_rng(33).random((n, 1)) < 0.7).astype(np.float32)
    p, y, m = T(sets[0][0]), T(sets[0][1]), T(m0)
    ops.auc_sorted(p, y, seg=seg, mask=m, return_counts=True)  # (the workspace of this shape exists before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        auc, counts = ops.auc_sorted(p, y, seg=seg, mask=m, return_counts=True)
    for pred_h, y_h in sets[1:]:
        p.copy_(T(pred_h))
        y.copy_(T(y_h))
        g.replay()
        torch.cuda.synchronize()
        got_auc, got_counts = auc.cpu().numpy().copy(), counts.cpu().numpy().copy()
        eager = run(ops, T(pred_h), T(y_h), seg=seg, mask=T(m0))
        assert np.array_equal(got_counts, eager[1])
        assert np.array_equal(got_auc.view(np.int64), eager[0].view(np.int64))
        check(pred_h, y_h, got_auc, got_counts, seg=seg, mask=m0, sklearn=False)


def test_bad_arguments_are_refused_without_a_launch(ops):
    from mmlrec_amd import _lib as L
    lib = L.load()
    n, cols = 1000, 2
    p = torch.rand(n, cols, device=dev())
    y = (p > 0.5).float()
    m = torch.ones(n, 3, device=dev())
    need = lib.mml_auc_sorted_workspace_bytes(n, cols, 0)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=dev())
    out = torch.full((1, cols), -7.0, dtype=torch.float64, device=dev())
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    stream = torch.cuda.current_stream().cuda_stream

    def call(n_=n, cols_=cols, mask=None, mask_cols=0, ws_bytes=need):
        return lib.mml_auc_sorted(p.data_ptr(), cols, y.data_ptr(), cols, None if mask is None else mask.data_ptr(), 3,
                                  mask_cols, n_, cols_, 0, ws.data_ptr(), ws_bytes, out.data_ptr(), None,
                                  status.data_ptr(), stream)

    ERR_ARG = -1
    assert call(ws_bytes=need - 1) == ERR_ARG                    # short workspace
    assert call(mask=m, mask_cols=3) == ERR_ARG                  # mask_cols not in {1, cols}
    assert call(n_=1 << 30, cols_=2) == ERR_ARG                  # n * cols == 2^31
    assert lib.mml_auc_sorted_workspace_bytes(1 << 30, 2, 0) < 0
    assert call(n_=0) == 0                                       # n == 0 is MML_OK
    torch.cuda.synchronize()
    assert (out == -7.0).all() and int(status.item()) == 0      # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert not (out == -7.0).any()
    with pytest.raises(L.MMLError):
        ops.auc_sorted(p, y, mask=m)
