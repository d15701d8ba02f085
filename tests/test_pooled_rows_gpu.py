"""The pooled-row kernels in isolation (mml_gather_pool_fwd, mml_scatter_pool_bwd, mml_index_unique_pool) against a
float64 numpy restatement of the reference's varlen_embedding_lookup + SequencePoolingLayer written in this file.

Grid: E in {4, 8, 16} x maxlen in {1, 5, 20, 64, 256} x B in {1, 64, 1000, 65 536} x {Zipf, uniform} ids -- the full
cross product, 120 cases.  Every case holds two single-valued fields (one on a 50-row table of its own, one SHARING its
table with the first pooled field) and three dense columns beside its pooled fields.  While B * maxlen <= 1.4 M a case
carries all six (combiner, mode) pairs at once -- sum / mean / max x mask / length.  Beyond that (B = 65 536 with
maxlen 64 or 256: up to 16.8 M lookups per field, whose float64 restatement on the host is what takes the time) a case
carries ONE pooled field, and the six pairs rotate over those twelve cases so that each pair runs twice there.

Bounds (none of them taken from what the kernels give):
  * single-valued blocks, dense columns and max blocks are copies / selections: np.array_equal, the all-padded
    float32(row - 1e9) included;
  * a sum block lies within maxlen * 2^-24 * sum_t |row_t[e]| of the float64 sum, the worst case of ANY fp32 summation
    order; a mean block within that bound / n_valid plus 2^-24 |result| for the one division; n_valid = 0 gives exact 0;
  * table gradients: rel < 1e-4 and elem_rel <= 1 (the definitions of tests/test_models_gpu.py) against float64;
    rows no valid position names are bitwise 0;
  * the touched list, the `seen` bitmaps and the row marks equal the set of valid rows exactly (per TABLE: the union
    over the fields that share it).
max with a length column has no reference behaviour (the reference raises); the kernels implement the masked max of
include/mmlrec.h and it is checked against this file's restatement only.
"""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-4
U = 2.0 ** -24
PAIRS = [("mean", False), ("sum", True), ("max", False), ("mean", True), ("sum", False), ("max", True)]
ES, TS, BS, DISTS = (4, 8, 16), (1, 5, 20, 64, 256), (1, 64, 1000, 65536), ("zipf", "uniform")
BIG = 1_400_000


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def elem_rel(a, b, floor=1e-5):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    return (np.abs(a - b) / (RTOL * np.abs(b) + floor * scale)).max()


def draw_ids(rng, dist, V, shape, lo):
    if dist == "zipf":
        return np.minimum(rng.zipf(1.3, size=shape) - 1 + lo, V - 1).astype(np.int64)
    return rng.integers(lo, V, size=shape, dtype=np.int64)


class Case:
    """X, tables and the field lists of one grid point.  Tables: 0 = 50 rows (single-valued field 0), 1 = shared by
    single-valued field 1 and pooled field 0, 2.. = one per further pooled field."""

    def __init__(self, E, T, B, dist, pairs, seed, V=5000):
        rng = np.random.default_rng(seed)
        self.E, self.T, self.B, self.pairs = E, T, B, pairs
        P = len(pairs)
        self.vocab = [50, V] + [V + 37 * p for p in range(1, P)]
        self.tables = [(rng.standard_normal((v, E)) * 0.1).astype(np.float32) for v in self.vocab]
        ncols = 2 + P * T + P + 3
        X = np.zeros((B, ncols), np.float32)
        X[:, 0] = rng.integers(0, 50, B)
        X[:, 1] = draw_ids(rng, dist, V, B, 0)
        self.singles = [(0, 0), (1, 1)]
        self.pooled = []  # (col0, T, combiner, table, len_col or None)
        self.ids, self.valid = [], []
        for p, (comb, use_len) in enumerate(pairs):
            c0, tb = 2 + p * T, (1 if p == 0 else 1 + p)
            Vp = self.vocab[tb]
            n = rng.integers(0, T + 1, B)  # lengths uniform in [0, maxlen]: length-0 (all padded) samples included
            pos = np.arange(T)[None, :]
            if use_len:
                ids = draw_ids(rng, dist, Vp, (B, T), 0)  # id 0 is an ordinary row; ids beyond the length stay in X
                lc = 2 + P * T + p
                ln = n.astype(np.float32)
                ln[rng.random(B) < 0.05] = T + 3  # a length above maxlen acts like maxlen
                ln[rng.random(B) < 0.05] = -2     # a length <= 0 like 0
                X[:, lc] = ln
                valid = pos < np.clip(ln.astype(np.int64), 0, T)[:, None]
            else:
                ids = draw_ids(rng, dist, Vp, (B, T), 1)
                ids[pos >= n[:, None]] = 0  # left-packed ...
                hole = rng.random(B) < 0.25  # ... and some sequences with a padded slot in the middle
                ids[hole, rng.integers(0, T, int(hole.sum()))] = 0
                lc = None
                valid = ids != 0
            if B >= 64:  # rows 1 and V - 1 forced to appear
                ids[0, 0], ids[1, 0] = 1, Vp - 1
                if use_len:
                    X[0, lc] = X[1, lc] = max(1, T // 2)
                    valid[0] = pos[0] < max(1, T // 2)
                    valid[1] = pos[0] < max(1, T // 2)
                else:
                    valid = ids != 0
            X[:, c0:c0 + T] = ids
            self.pooled.append((c0, T, comb, tb, lc))
            self.ids.append(ids)
            self.valid.append(valid)
        self.dense_col0, self.nd = ncols - 3, 3
        X[:, self.dense_col0:] = rng.standard_normal((B, 3))
        self.X = X
        self.d_out = rng.standard_normal((B, (2 + P) * E)).astype(np.float32)

    # ---- float64 restatement ----------------------------------------------------------------------------------
    def forward64(self, p):
        """(value [B, E] float64 -- float32-exact for max --, bound [B, E], argmax [B, E] or None, n_valid [B])"""
        c0, T, comb, tb, lc = self.pooled[p]
        ids, valid, tab = self.ids[p], self.valid[p], self.tables[tb]
        n = valid.sum(1)
        B, E = self.B, self.E
        val = np.zeros((B, E))
        bound = np.zeros((B, E))
        arg = None if comb != "max" else np.zeros((B, E), np.int64)
        step = max(1, (1 << 21) // (T * E))
        for s in range(0, B, step):
            r32 = tab[ids[s:s + step]]  # [b, T, E]
            v = valid[s:s + step, :, None]
            if comb == "max":
                h = np.where(v, r32, (r32 - np.float32(1e9)).astype(np.float32))
                val[s:s + step] = h.max(1)
                arg[s:s + step] = h.argmax(1)  # the first (lowest) position that attains the maximum
            else:
                r = r32.astype(np.float64) * v
                val[s:s + step] = r.sum(1)
                bound[s:s + step] = T * U * np.abs(r).sum(1)
        if comb == "mean":
            div = (n.astype(np.float32) + np.float32(1e-8)).astype(np.float64)[:, None]
            val = val / div
            bound = bound / np.maximum(n, 1)[:, None] + U * np.abs(val)
        return val, bound, arg, n

    def grads64(self, args):
        """float64 table gradients of every table; args[p] = the argmax the backward is to follow (max fields)."""
        E, B = self.E, self.B
        G = [np.zeros((v, E)) for v in self.vocab]
        d = self.d_out.astype(np.float64)
        for f, (c, tb) in enumerate(self.singles):
            rows = self.X[:, c].astype(np.int64)
            for e in range(E):
                G[tb][:, e] += np.bincount(rows, weights=d[:, f * E + e], minlength=self.vocab[tb])
        for p, (c0, T, comb, tb, lc) in enumerate(self.pooled):
            ids, valid = self.ids[p], self.valid[p]
            blk = d[:, (2 + p) * E:(3 + p) * E]
            V = self.vocab[tb]
            if comb == "max":
                ar = np.arange(B)
                for e in range(E):
                    t = args[p][:, e]
                    ok = valid[ar, t]  # an all-padded sample has no valid position: no gradient
                    G[tb][:, e] += np.bincount(ids[ar, t][ok], weights=blk[ok, e], minlength=V)
                continue
            if comb == "mean":
                n = valid.sum(1)
                blk = blk / (n.astype(np.float32) + np.float32(1e-8)).astype(np.float64)[:, None]
            bi, ti = np.nonzero(valid)
            rows = ids[bi, ti]
            for e in range(E):
                G[tb][:, e] += np.bincount(rows, weights=blk[bi, e], minlength=V)
        return G

    def valid_rows(self):
        """per table: the sorted distinct rows some VALID position (or single-valued field) names"""
        sets = [set() for _ in self.vocab]
        for c, tb in self.singles:
            sets[tb].update(np.unique(self.X[:, c].astype(np.int64)).tolist())
        for p, (c0, T, comb, tb, lc) in enumerate(self.pooled):
            sets[tb].update(np.unique(self.ids[p][self.valid[p]]).tolist())
        return [np.array(sorted(s), np.int64) for s in sets]

    # ---- device side ------------------------------------------------------------------------------------------
    def fields(self):
        from mmlrec_amd import ops
        return [ops.PooledField(c0, T, comb, tb, lc) for c0, T, comb, tb, lc in self.pooled]


def bookkeeping(case, dev):
    vocab = case.vocab
    seen = [torch.zeros((v + 31) // 32, dtype=torch.int32, device=dev) for v in vocab]
    rowbase = np.concatenate([[0], np.cumsum(vocab)]).tolist()
    touched = torch.full((sum(vocab),), -1, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    return seen, rowbase, touched, count


def check_sets(case, seen, rowbase, touched, count, marks=None):
    want = case.valid_rows()
    glob = np.concatenate([w + rowbase[t] for t, w in enumerate(want)])
    n = int(count.item())
    assert n == len(glob), (n, len(glob))
    assert np.array_equal(np.sort(touched[:n].cpu().numpy().astype(np.int64)), np.sort(glob))
    for t, w in enumerate(want):
        bits = np.unpackbits(seen[t].cpu().numpy().view(np.uint8), bitorder="little")[:case.vocab[t]]
        assert np.array_equal(np.nonzero(bits)[0], w), f"seen bitmap of table {t}"
    if marks is not None:
        assert int(marks.count_nonzero()) == 0  # the compaction consumed the marks


def grid():
    big = 0
    for E, T, B, dist in itertools.product(ES, TS, BS, DISTS):
        if B * T <= BIG:
            pairs = tuple(PAIRS)
        else:
            pairs = (PAIRS[big % len(PAIRS)],)
            big += 1
        yield pytest.param(E, T, B, dist, pairs, id=f"E{E}-T{T}-B{B}-{dist}-{'all' if len(pairs) > 1 else pairs[0][0] + ('_len' if pairs[0][1] else '_mask')}")


@pytest.mark.parametrize("E,T,B,dist,pairs", list(grid()))
def test_pooled_gather_scatter(E, T, B, dist, pairs):
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import ops
    dev = torch.device("cuda:0")
    case = Case(E, T, B, dist, pairs, seed=E * 100003 + T * 1009 + B + (dist == "zipf"))
    P = len(pairs)
    tabs = [torch.from_numpy(t).to(dev) for t in case.tables]
    X = torch.from_numpy(case.X).to(dev)
    status = ops.new_status(dev)
    pooled = case.fields()
    # ---- forward
    out, argmax, wg = ops.gather_pool_fwd(tabs, X, case.singles, pooled, case.dense_col0, case.nd, wgmax=True,
                                          status=status)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    o = out.cpu().numpy()
    assert o.shape == (B, (2 + P) * E + 3)
    for f, (c, tb) in enumerate(case.singles):
        assert np.array_equal(o[:, f * E:(f + 1) * E], case.tables[tb][case.X[:, c].astype(np.int64)])
    assert np.array_equal(o[:, (2 + P) * E:], case.X[:, case.dense_col0:])
    args = {}
    for p, (c0, T_, comb, tb, lc) in enumerate(case.pooled):
        got = o[:, (2 + p) * E:(3 + p) * E]
        val, bound, arg, n = case.forward64(p)
        if comb == "max":
            assert np.array_equal(got, val.astype(np.float32)), (p, comb)
            some = n > 0
            ga = argmax.cpu().numpy()[:, p * E:(p + 1) * E].astype(np.int64)
            assert np.array_equal(ga[some], arg[some]), "arg-max: the lowest position wins a tie"
            if (~some).any():  # all padded: float32(row - 1e9), -1e9 for any sane weight
                assert np.all(got[~some] == np.float32(-1e9))
            args[p] = arg
        else:
            err = np.abs(got.astype(np.float64) - val)
            print(f"[pooled fwd] E={E} T={T} B={B} {dist} {comb} len={lc is not None}: "
                  f"max err/bound = {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
            assert np.all(err <= bound), (p, comb, float((err - bound).max()))
            assert np.all(got[n == 0] == 0.0)
    w = wg.cpu().numpy().ravel()
    assert not np.isnan(w).any()  # every workgroup wrote its word
    assert float(w.max()) == float(np.abs(o).max())
    # per segment of the grid (include/mmlrec.h, tests/test_pooled_cpu.py: segment 0 = single-valued blocks + dense
    # columns, 256 sixteen-byte pieces per workgroup; segment 1 + p = pooled field p)
    e4 = E // 4
    n0 = -(-B * (2 * e4 + 1) // 256)
    G = e4
    while G < 64 and G < T * e4:
        G *= 2
    per_block = (256 // G) * (4 if T * e4 <= G else 1)
    assert w.size == n0 + P * -(-B // per_block)
    a0 = np.abs(np.concatenate([o[:, :2 * E], o[:, (2 + P) * E:]], 1))
    assert float(w[:n0].max()) == float(a0.max())
    per_row = a0.max(1)  # a workgroup of segment 0 covers whole or partial rows: its word is bounded by its rows' maxima
    for blk in range(min(n0, 64)):
        r0, r1 = blk * 256 // (2 * e4 + 1), min(B - 1, (blk * 256 + 255) // (2 * e4 + 1))
        assert w[blk] <= per_row[r0:r1 + 1].max()
    nb = -(-B // per_block)
    for p in range(P):
        blockmax = np.abs(o[:, (2 + p) * E:(3 + p) * E]).max(1)
        pad = np.zeros(nb * per_block)
        pad[:B] = blockmax
        assert np.array_equal(w[n0 + p * nb:n0 + (p + 1) * nb], pad.reshape(nb, per_block).max(1).astype(np.float32))
    # ---- backward, with the touched list built from row marks
    gtabs = [torch.zeros_like(t) for t in tabs]
    seen, rowbase, touched, count = bookkeeping(case, dev)
    marks = torch.zeros(ops.marks_bytes(case.vocab), dtype=torch.uint8, device=dev)
    d_out = torch.from_numpy(case.d_out).to(dev)
    ops.scatter_pool_bwd(gtabs, X, case.singles, pooled, d_out, argmax=argmax, seen=seen, rowbase=rowbase,
                         touched=touched, touched_count=count, status=status, marks=marks)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    G = case.grads64(args)
    want = case.valid_rows()
    for t, g64 in enumerate(G):
        got = gtabs[t].cpu().numpy()
        r, er = rel(got, g64), elem_rel(got, g64)
        print(f"[pooled bwd] E={E} T={T} B={B} {dist} table {t}: rel={r:.3g} elem_rel={er:.3g}")
        assert r < RTOL and er <= 1.0, (t, r, er)
        idle = np.ones(case.vocab[t], bool)
        idle[want[t]] = False
        assert not got[idle].view(np.uint32).any(), "a row no valid position names must stay bitwise 0"
    check_sets(case, seen, rowbase, touched, count, marks)
    # ---- the index-only pass returns the same set
    seen2, _, touched2, count2 = bookkeeping(case, dev)
    ops.index_unique_pool(case.vocab, E, X, case.singles, pooled, seen2, rowbase, touched2, count2, status=status,
                          marks=marks)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    check_sets(case, seen2, rowbase, touched2, count2, marks)


@pytest.mark.parametrize("E", ES)
def test_bookkeeping_without_marks_and_marks_alone(E):
    """The other two bookkeeping forms of mml_scatter_bwd: bitmaps + list without a mark map (the fold kernel sets the
    bits itself), and a mark map without a list (the bytes stay set for the marked dense update)."""
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import ops
    dev = torch.device("cuda:0")
    case = Case(E, 20, 1000, "zipf", tuple(PAIRS), seed=77 + E)
    tabs = [torch.from_numpy(t).to(dev) for t in case.tables]
    X = torch.from_numpy(case.X).to(dev)
    pooled = case.fields()
    _, argmax, _ = ops.gather_pool_fwd(tabs, X, case.singles, pooled, case.dense_col0, case.nd)
    d_out = torch.from_numpy(case.d_out).to(dev)
    want = case.valid_rows()
    # bitmaps + list, no marks
    gt = [torch.zeros_like(t) for t in tabs]
    seen, rowbase, touched, count = bookkeeping(case, dev)
    ops.scatter_pool_bwd(gt, X, case.singles, pooled, d_out, argmax=argmax, seen=seen, rowbase=rowbase,
                         touched=touched, touched_count=count)
    check_sets(case, seen, rowbase, touched, count)
    seen, rowbase, touched, count = bookkeeping(case, dev)
    ops.index_unique_pool(case.vocab, E, X, case.singles, pooled, seen, rowbase, touched, count)
    check_sets(case, seen, rowbase, touched, count)
    # marks alone
    gt2 = [torch.zeros_like(t) for t in tabs]
    marks = torch.zeros(ops.marks_bytes(case.vocab), dtype=torch.uint8, device=dev)
    ops.scatter_pool_bwd(gt2, X, case.singles, pooled, d_out, argmax=argmax, marks=marks)
    m = marks.cpu().numpy()
    base = 0
    for t, v in enumerate(case.vocab):
        assert np.array_equal(np.nonzero(m[base:base + v])[0], want[t]), f"marks of table {t}"
        assert not m[base + v:base + 32 * ((v + 31) // 32)].any()
        base += 32 * ((v + 31) // 32)


@pytest.mark.parametrize("use_len", [False, True])
def test_status_only_at_valid_positions(use_len):
    """An out-of-range id at a valid position sets the status bit; the same id at a padded position does not (and is
    not used as an address)."""
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import ops
    dev = torch.device("cuda:0")
    E, T, B, V = 8, 6, 32, 100
    tab = torch.randn(V, E, device=dev)
    for where, expect in (("padded", 0), ("valid", 2), ("valid_negative", 1)):
        X = np.zeros((B, T + 1), np.float32)
        X[:, :3] = 5  # three valid positions (ids != 0, length 3)
        X[:, T] = 3
        if use_len:
            X[7, 4 if where == "padded" else 1] = -3 if where == "valid_negative" else V + 50
        elif where == "padded":
            continue  # mask mode: a padded position holds id 0 by definition, there is no other id to place there
        else:
            X[7, 1] = -3 if where == "valid_negative" else V + 50
        Xd = torch.from_numpy(X).to(dev)
        pf = [ops.PooledField(0, T, "sum", 0, T if use_len else None)]
        status = ops.new_status(dev)
        ops.gather_pool_fwd([tab], Xd, [], pf, status=status)
        assert int(status.item()) == expect, ("gather", where)
        status.zero_()
        g = [torch.zeros_like(tab)]
        ops.scatter_pool_bwd(g, Xd, [], pf, torch.ones(B, E, device=dev), status=status)
        assert int(status.item()) == expect, ("scatter", where)
        status.zero_()
        seen = [torch.zeros((V + 31) // 32, dtype=torch.int32, device=dev)]
        touched = torch.zeros(V, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        marks = torch.zeros(ops.marks_bytes([V]), dtype=torch.uint8, device=dev)
        ops.index_unique_pool([V], E, Xd, [], pf, seen, [0, V], touched, count, status=status, marks=marks)
        assert int(status.item()) == expect, ("index_unique", where)
        assert sorted(touched[:int(count.item())].cpu().tolist()) == [5]


def test_shapes_outside_the_contract_are_refused():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import ops, _lib
    dev = torch.device("cuda:0")
    X = torch.zeros(4, 300, device=dev)
    with pytest.raises(_lib.MMLError):  # E = 12
        ops.gather_pool_fwd([torch.zeros(10, 12, device=dev)], X, [], [ops.PooledField(0, 4, "sum", 0)])
    with pytest.raises(_lib.MMLError):  # maxlen 257
        ops.gather_pool_fwd([torch.zeros(10, 8, device=dev)], X, [], [ops.PooledField(0, 257, "sum", 0)])
    with pytest.raises(_lib.MMLError):  # table index out of range
        ops.gather_pool_fwd([torch.zeros(10, 8, device=dev)], X, [], [ops.PooledField(0, 4, "sum", 1)])
    with pytest.raises(_lib.MMLError):  # more pooled fields than the descriptor holds
        ops.gather_pool_fwd([torch.zeros(10, 8, device=dev)], X, [],
                            [ops.PooledField(0, 4, "sum", 0)] * (_lib.MAX_POOLED + 1))
    with pytest.raises(_lib.MMLError):  # X narrower than the columns the field reads
        ops.gather_pool_fwd([torch.zeros(10, 8, device=dev)], X[:, :3].contiguous(), [], [ops.PooledField(0, 4, "sum", 0)])
