"""mml_opt_tensor.warm_rows: the marked streaming table update passes over the rows whose moments are still zero and whose
gradient is unmarked, without reading them.  Every case compares bit for bit against the same steps without the map (the
update of every row), from the same state and the same gradient bits; the streaming launch exists from 2^24 parameters
up, so one table of (1 << 24) // E + 37 rows is the smallest shape."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 3000


@pytest.fixture(scope="module")
def env():
    import torch
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, ops
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch, L, ops


def _index_sets(rng, V, steps, only_first=()):
    """Row sets of `steps` batches: each holds row 0 and the last row; the rows of `only_first` are in the first set only."""
    out = []
    for s in range(steps):
        idx = np.r_[0, V - 1, rng.integers(0, V, B - 2 - len(only_first))]
        idx = idx[~np.isin(idx, only_first)]
        if s == 0:
            idx = np.r_[idx, only_first]
        out.append(idx.astype(np.int64))
    return out


def _entry(kind, p, g, m, v, marks, warm, det=None):
    return (p, g, m if kind != "sgd" else None, v if kind == "adam" else None, None, None, marks, det, warm)


@functools.lru_cache(maxsize=None)
def _cold_start(kind, E, cap):
    """Three steps from zero moments and a zero map against the same steps without a map; everything the issue lists is
    asserted here after every step.  Returns the tracked row's (p, m, v) after every step of the run with the map."""
    import torch
    from mmlrec_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31 + E)
    V = (1 << 24) // E + 37
    track = 123457                                # touched in step 1 and never again
    g_ = torch.Generator(device=dev).manual_seed(E)
    p = torch.randn(V, E, generator=g_, device=dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    pr, mr, vr = p.clone(), m.clone(), v.clone()
    grads, grads_r = torch.zeros_like(p), torch.zeros_like(p)
    marks = torch.zeros(ops.marks_bytes([V]), dtype=torch.uint8, device=dev)
    marks_r = torch.zeros_like(marks)
    warm = torch.zeros(V, dtype=torch.uint8, device=dev)
    union = torch.zeros(V, dtype=torch.bool, device=dev)
    snaps = []
    for step, idx in enumerate(_index_sets(rng, V, 3, only_first=[track]), 1):
        X = torch.from_numpy(idx.astype(np.float32)).to(dev).view(-1, 1)
        assert torch.equal(X.view(-1).long().cpu(), torch.from_numpy(idx))       # (row ids below 2^24 are exact floats)
        d = torch.from_numpy(rng.standard_normal((len(idx), E)).astype(np.float32)).to(dev)
        ops.scatter_bwd([grads], X, [0], d, marks=marks)
        grads_r.copy_(grads)                                                     # the same gradient bits in both runs
        marks_r.copy_(marks)
        union[torch.from_numpy(idx).to(dev)] = True
        assert int(marks[:V].sum()) == len(np.unique(idx))
        hyper = ops.make_hyper(kind, 0.01, step=step, zero_grad=True, max_blocks=cap)
        ops.opt_step_dense([_entry(kind, p, grads, m, v, marks[:V], warm)], hyper)
        ops.opt_step_dense([_entry(kind, pr, grads_r, mr, vr, marks_r[:V], None)], hyper)
        assert torch.equal(p.view(torch.int32), pr.view(torch.int32)), (kind, E, step)
        assert torch.equal(m.view(torch.int32), mr.view(torch.int32)), (kind, E, step)
        if kind == "adam":
            assert torch.equal(v.view(torch.int32), vr.view(torch.int32)), (kind, E, step)
        assert torch.equal(warm, union.to(torch.uint8)), (kind, E, step)         # exactly the rows marked so far
        assert int(marks.max()) == 0 and int(marks_r.max()) == 0
        assert float(grads.abs().max()) == 0.0 and float(grads_r.abs().max()) == 0.0
        snaps.append((p[track].clone(), m[track].clone(), v[track].clone()))
    assert float(m.abs().max()) > 0.0                                            # (the steps did move something)
    return snaps


@pytest.mark.parametrize("kind,E", [("adam", 8), ("adam", 4), ("rmsprop", 16), ("adagrad", 8)])
def test_cold_start_is_exact(env, kind, E):
    _cold_start(kind, E, 1 << 20)


def test_warm_rows_keep_moving(env):
    """A row touched in step 1 only: its moments decay and Adam keeps moving it in steps 2 and 3 (equal to the run
    without the map: asserted for every row inside _cold_start)."""
    torch, _, _ = env
    s = _cold_start("adam", 8, 1 << 20)
    for a, b in ((s[0], s[1]), (s[1], s[2])):
        for which in range(3):
            assert bool((a[which] != b[which]).all()), which


def test_deferred_totals(env):
    """Form 4: the totals of the deterministic scatter are still in acc64 -- the same bits with and without the map, and
    the totals, marks and gradients are zero afterwards."""
    torch, L, ops = env
    dev = torch.device("cuda:0")
    E = 8
    V = (1 << 24) // E + 37
    rng = np.random.default_rng(5)
    sets = _index_sets(rng, V, 3)
    ds = [rng.standard_normal((len(i), E)).astype(np.float32) for i in sets]
    shift = ops.scatter_det_shift(B)
    finals = []
    for with_map in (True, False):
        g_ = torch.Generator(device=dev).manual_seed(77)
        p = torch.randn(V, E, generator=g_, device=dev)
        m, v, grads = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
        acc = torch.zeros(V, E, dtype=torch.int64, device=dev)
        marks = torch.zeros(ops.marks_bytes([V]), dtype=torch.uint8, device=dev)
        warm = torch.zeros(V, dtype=torch.uint8, device=dev) if with_map else None
        slot = ops.amax_slots(1, dev)[0]
        for step, (idx, d) in enumerate(zip(sets, ds), 1):
            X = torch.from_numpy(idx.astype(np.float32)).to(dev).view(-1, 1)
            dd = torch.from_numpy(d).to(dev)
            slot.zero_()
            ops.amax_batch([(dd, slot)])
            ops.scatter_bwd_det([grads], X, [0], dd, [acc], marks, amax_slot=slot, clear_marks=False, amax_supplied=True,
                                defer_totals=True)
            assert int(acc.abs().max()) > 0 and int(marks.max()) == 1
            hyper = ops.make_hyper("adam", 0.01, step=step, zero_grad=True, max_blocks=1 << 20)
            ops.opt_step_dense([_entry("adam", p, grads, m, v, marks[:V], warm, det=(acc, slot, shift))], hyper)
            assert int(acc.abs().max()) == 0 and int(marks.max()) == 0 and float(grads.abs().max()) == 0.0
        if with_map:
            want = np.zeros(V, bool)
            want[np.concatenate(sets)] = True
            assert np.array_equal(warm.cpu().numpy().astype(bool), want)
        finals.append((p, m, v))
        del acc, grads
    for a, b in zip(*finals):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(finals[0][1].abs().max()) > 0.0


@pytest.mark.parametrize("cap", [0, 1 << 20, 300])
def test_one_launch_over_many_tables(env, cap):
    """Seven tables (a one-row table, row counts that are no multiple of 32) in one marked launch, with a workgroup cap
    and without: bitwise the per-table plain dense steps, warm exactly on the rows marked so far."""
    torch, L, ops = env
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(21)
    E = 8
    vocab = [(1 << 24) // E + 5, 1, 37, 300000, 4097, 64, 250001]
    F = len(vocab)
    g = torch.Generator(device="cpu").manual_seed(3)
    tabs = [torch.randn(v, E, generator=g).to(dev) for v in vocab]
    ref = [t.clone() for t in tabs]
    st = [[torch.zeros(v, E, device=dev) for v in vocab] for _ in range(2)]
    st_ref = [[torch.zeros(v, E, device=dev) for v in vocab] for _ in range(2)]
    grads = [torch.zeros(v, E, device=dev) for v in vocab]
    marks = torch.zeros(ops.marks_bytes(vocab), dtype=torch.uint8, device=dev)
    base = np.concatenate([[0], np.cumsum([(v + 31) // 32 * 32 for v in vocab])]).tolist()
    warm = [torch.zeros(v, dtype=torch.uint8, device=dev) for v in vocab]
    union = [np.zeros(v, bool) for v in vocab]
    for step in (1, 2, 3):
        X = np.stack([np.r_[0, vocab[f] - 1, rng.integers(0, vocab[f], B - 2)] for f in range(F)], 1).astype(np.float32)
        d_out = torch.from_numpy(rng.standard_normal((B, F * E)).astype(np.float32)).to(dev)
        ops.scatter_bwd(grads, torch.from_numpy(X).to(dev), list(range(F)), d_out, marks=marks)
        grads_ref = [g_.clone() for g_ in grads]
        hyper = ops.make_hyper("adam", 0.01, step=step, zero_grad=True, max_blocks=cap)
        ops.opt_step_dense([_entry("adam", tabs[f], grads[f], st[0][f], st[1][f], marks[base[f]:base[f] + vocab[f]],
                                   warm[f]) for f in range(F)], hyper)
        plain = ops.make_hyper("adam", 0.01, step=step, zero_grad=True)
        for f in range(F):
            ops.opt_step_dense([(ref[f], grads_ref[f], st_ref[0][f], st_ref[1][f])], plain)
        for f in range(F):
            union[f][X[:, f].astype(np.int64)] = True
            assert torch.equal(tabs[f], ref[f]), (step, f)
            assert torch.equal(st[0][f], st_ref[0][f]) and torch.equal(st[1][f], st_ref[1][f]), (step, f)
            assert float(grads[f].abs().max()) == 0.0
            assert np.array_equal(warm[f].cpu().numpy().astype(bool), union[f]), (step, f)
        assert int(marks.max()) == 0


def test_all_ones_map_over_nonzero_moments_is_the_plain_step(env):
    """A map that says 'warm' everywhere hides nothing: non-zero moments, every row updated as without a map."""
    torch, L, ops = env
    dev = torch.device("cuda:0")
    E = 8
    V = (1 << 24) // E + 37
    g_ = torch.Generator(device=dev).manual_seed(9)
    p = torch.randn(V, E, generator=g_, device=dev)
    m = torch.randn(V, E, generator=g_, device=dev) * 0.1
    v = torch.rand(V, E, generator=g_, device=dev)
    pr, mr, vr = p.clone(), m.clone(), v.clone()
    grads, grads_r = torch.zeros_like(p), torch.zeros_like(p)
    marks = torch.zeros(ops.marks_bytes([V]), dtype=torch.uint8, device=dev)
    marks_r = torch.zeros_like(marks)
    warm = torch.ones(V, dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(2)
    idx = _index_sets(rng, V, 1)[0]
    X = torch.from_numpy(idx.astype(np.float32)).to(dev).view(-1, 1)
    d = torch.from_numpy(rng.standard_normal((len(idx), E)).astype(np.float32)).to(dev)
    ops.scatter_bwd([grads], X, [0], d, marks=marks)
    grads_r.copy_(grads)
    marks_r.copy_(marks)
    hyper = ops.make_hyper("adam", 0.01, step=4, zero_grad=True, max_blocks=1 << 20)
    ops.opt_step_dense([_entry("adam", p, grads, m, v, marks[:V], warm)], hyper)
    ops.opt_step_dense([_entry("adam", pr, grads_r, mr, vr, marks_r[:V], None)], hyper)
    for a, b in ((p, pr), (m, mr), (v, vr)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert int(warm.min()) == 1 and int(marks.max()) == 0 and float(grads.abs().max()) == 0.0


def test_the_map_needs_marks_and_no_regulariser(env):
    torch, L, ops = env
    dev = torch.device("cuda:0")
    V, E = (1 << 24) // 8 + 37, 8
    p = torch.zeros(V, E, device=dev)
    g, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    marks = torch.zeros(V, dtype=torch.uint8, device=dev)
    warm = torch.zeros(V, dtype=torch.uint8, device=dev)
    hyper = ops.make_hyper("adam", 0.01, step=1, max_blocks=1 << 20)
    with pytest.raises(L.MMLError):
        ops.opt_step_dense([(p, g, m, v, None, None, None, None, warm)], hyper)              # no marks
    with pytest.raises(L.MMLError):
        ops.opt_step_dense([(p, g, m, v, (0.0, 1e-4), None, marks, None, warm)], hyper)      # a regulariser


# ---- whole steps ------------------------------------------------------------------------------------------------------
STEP_B = 4096
STEP_VOCAB = [(1 << 21) + 5, 50, 7]       # E = 8: the first table alone reaches 2^24 parameters (the streaming launch)


def _model(torch, W):
    from mmlrec_amd import model as M
    dev = torch.device("cuda:0")
    cfg, _, _, _ = W.workload("sharedbottom_ml")
    cfg["model_config"].update(emb=8, table_update="dense_exact")
    cols = [M.SparseFeat("s%d" % i, v, embedding_dim=8) for i, v in enumerate(STEP_VOCAB)]
    torch.manual_seed(0)
    model = M.SharedBottom(cols, device="cpu", config=cfg).to(dev)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():  # (the reference's 1e-4 initialisation gives gradients at Adam's eps)
        for n, p in model.named_parameters():
            if p.dim() == 2:
                scale = 0.05 if n.startswith("embedding") else (2.0 / p.shape[1]) ** 0.5
                p.copy_((torch.randn(p.shape, generator=g) * scale).to(dev))
    model.scatter_mode = "deterministic"
    model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
    model.train()
    return model, cfg


def _table_launches(L, runner):
    """Per mml_opt_step_dense entry of the step that carries gradient marks: does every tensor of it carry a warm map?"""
    lib = L.load()
    out = []
    for c in runner.opt_calls:
        if c[0] is lib.mml_opt_step_dense and any(c[1][0][k].grad_marks for k in range(c[1][1])):
            out.append(all(bool(c[1][0][k].warm_rows) for k in range(c[1][1])))
    return out


def _feed(torch, W, cfg, runner, seed):
    X, y = W.synth_batch(STEP_VOCAB, 0, STEP_B, W.num_tasks(cfg), seed=seed)
    runner.plan.X.copy_(X.cuda())
    runner.plan.y.copy_(y.cuda())
    runner.run()


def _final(torch, model):
    torch.cuda.synchronize()
    opt = model.optimizer()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    mom = {n: tuple(s.clone() for s in opt.state[n]) for n in opt.store.table_names}
    return sd, mom


def _same(torch, a, b):
    assert set(a[0]) == set(b[0]) and set(a[1]) == set(b[1])
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    for n in a[1]:
        for x, y in zip(a[1][n], b[1][n]):
            assert torch.equal(x, y), n


def test_whole_step_with_and_without_the_map(env, monkeypatch):
    """Four dense_exact steps with the deterministic scatter, with the map and with MMLREC_OPT_COLD_ROWS=0: state_dict()
    and the moments equal; the step's marked launch carries the map in the first run only."""
    torch, L, _ = env
    from mmlrec_amd import workloads as W
    finals = []
    for cold in (True, False):
        if cold:
            monkeypatch.delenv("MMLREC_OPT_COLD_ROWS", raising=False)
        else:
            monkeypatch.setenv("MMLREC_OPT_COLD_ROWS", "0")
        model, cfg = _model(torch, W)
        runner = model.train_step_runner(STEP_B, use_graph=True, split_dense=False)
        assert _table_launches(L, runner) == [cold]
        for i in range(4):
            _feed(torch, W, cfg, runner, 1 + i)
        finals.append(_final(torch, model))
        if cold:
            warm = model.optimizer().warm["embedding_dict.s0.weight"]
            assert 0 < int(warm.sum()) < 4 * STEP_B        # a few thousand of 2 M rows: the rest was never read
        del model, runner
    _same(torch, finals[0], finals[1])


def test_split_dense_step_between_dense_steps_marks_every_row_warm(env, monkeypatch):
    """dense_exact steps, a split-dense step (its row kernels write moments and know no map), dense_exact again -- equal to
    the same schedule that never had a map."""
    torch, L, _ = env
    from mmlrec_amd import workloads as W
    finals = []
    for cold in (True, False):
        if cold:
            monkeypatch.delenv("MMLREC_OPT_COLD_ROWS", raising=False)
        else:
            monkeypatch.setenv("MMLREC_OPT_COLD_ROWS", "0")
        model, cfg = _model(torch, W)
        dense = model.train_step_runner(STEP_B, use_graph=False, split_dense=False)
        assert _table_launches(L, dense) == [cold]
        for i in range(2):
            _feed(torch, W, cfg, dense, 1 + i)
        if cold:
            warm = model.optimizer().warm["embedding_dict.s0.weight"]
            assert 0 < int(warm.sum()) < 2 * STEP_B
        split = model.train_step_runner(STEP_B, use_graph=False, split_dense="force")
        assert split is not dense and split.split_dense
        if cold:
            assert int(warm.min()) == 1                    # from the moment the split step's call list exists
        _feed(torch, W, cfg, split, 3)
        dense = model.train_step_runner(STEP_B, use_graph=False, split_dense=False)
        for i in range(2):
            _feed(torch, W, cfg, dense, 4 + i)
        finals.append(_final(torch, model))
        del model, dense, split
    _same(torch, finals[0], finals[1])
