"""Parity at BASELINE.json's full sizes (AE-30: 12.49 M table rows, 1e7-row top table) through size-independent
properties plus one full-size step against the oracle: bit-exact gather on formula-defined tables, scatter checksums /
touched-row set, and a fused train step (dense-exact Adam over every row) vs oracle/mmlrec_oracle.py."""
import numpy as np
import pytest
import torch

from conftest import check_tables, check_update, randomize_he

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def W():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import workloads
    return workloads


def formula_table(v, e, salt):
    """Every element a distinct finite bit pattern in [1,2): any flipped bit or misplaced row is visible."""
    idx = torch.arange(v * e, dtype=torch.int64, device=dev())
    bits = ((idx * 2654435761 + salt * 40503) & 0x007FFFFF) | 0x3F800000
    return bits.to(torch.int32).view(torch.float32).view(v, e)


def test_gather_bit_exact_at_full_vocab(W):
    from mmlrec_amd import ops
    vocab, E, B = W.AE30_VOCAB, 8, 65536
    tabs = [formula_table(v, E, f) for f, v in enumerate(vocab)]
    X, _ = W.synth_batch(vocab, 0, B, 2, seed=3, dist="zipf")
    Xu, _ = W.synth_batch(vocab, 0, B, 2, seed=4, dist="uniform")
    X = torch.cat([X[:B // 2], Xu[:B // 2]])
    for f, v in enumerate(vocab):  # edge rows: first / last of every table, incl. 9 999 999
        X[0, f], X[1, f] = 0.0, float(v - 1)
    status = ops.new_status(dev())
    out = ops.gather_fwd(tabs, X.to(dev()), list(range(len(vocab))), status=status)
    ops.check_status(status)
    idx = X.long().to(dev())
    ref = torch.cat([tabs[f][idx[:, f]] for f in range(len(vocab))], 1)  # plain indexing as the bit-level reference
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    # and against the closed form on the host for a sample of rows (independent of torch indexing on the device)
    b = np.array([0, 1, 17, B // 2, B - 1])
    for f in (0, 5, len(vocab) - 1):
        r = X[b, f].numpy().astype(np.int64)
        e = np.arange(E)
        bits = (((r[:, None] * E + e[None, :]) * 2654435761 + f * 40503) & 0x007FFFFF) | 0x3F800000
        got = out[b, f * E:(f + 1) * E].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, bits.astype(np.uint32))


def test_scatter_checksums_and_touched_rows_at_full_vocab(W):
    from mmlrec_amd import ops
    vocab, E, B = W.AE30_VOCAB, 8, 65536
    F = len(vocab)
    X, _ = W.synth_batch(vocab, 0, B, 2, seed=9, dist="zipf")
    Xd = X.to(dev())
    g = torch.randn(B, F * E, device=dev())
    gt = [torch.zeros(v, E, device=dev()) for v in vocab]
    seen = [torch.zeros((v + 31) // 32, dtype=torch.int32, device=dev()) for v in vocab]
    rowbase = np.concatenate([[0], np.cumsum(vocab)]).tolist()
    touched = torch.full((B * F,), -1, dtype=torch.int32, device=dev())
    count = torch.zeros(1, dtype=torch.int32, device=dev())
    ops.scatter_bwd(gt, Xd, list(range(F)), g, seen=seen, rowbase=rowbase, touched=touched, touched_count=count)
    # checksum of checksums: every gradient float lands in exactly one table row
    for f in range(F):
        col = g[:, f * E:(f + 1) * E].double().sum(0)
        tab = gt[f].double().sum(0)
        assert torch.allclose(col, tab, rtol=1e-5, atol=1e-3), f
    # per-row check against index_add on a mid-size table and the giant one
    for f in (0, 3, F - 1):
        ref = torch.zeros(vocab[f], E, dtype=torch.float64, device=dev())
        ref.index_add_(0, Xd[:, f].long(), g[:, f * E:(f + 1) * E].double())
        err = (gt[f].double() - ref).abs().max().item() / ref.abs().max().item()
        assert err < 1e-5, (f, err)
    # touched list == set of unique (field, row) pairs
    n = int(count.item())
    want = torch.cat([torch.unique(Xd[:, f].long()) + rowbase[f] for f in range(F)])
    got = torch.sort(touched[:n].long())[0]
    assert n == want.numel() and torch.equal(got, torch.sort(want)[0])
    # linearity: scattering 2*g on top gives 3x (exact powers of two keep fp32 exact up to summation order)
    ops.scatter_bwd(gt, Xd, list(range(F)), 2.0 * g)
    col = g[:, :E].double().sum(0) * 3
    assert torch.allclose(gt[0].double().sum(0), col, rtol=1e-5, atol=1e-3)


def test_full_size_fused_step_matches_oracle(W):
    """AE-30 at full vocabulary, B = 8192: forward loss, MLP update and the dense-exact Adam over all 12.49 M rows."""
    from oracle import mmlrec_oracle as orc
    model, cfg, vocab, dense = W.build_model("mmoe_ae30", dev(), table_update="dense_exact")
    names = [f.name for f in model._sparse_cols()]
    spec = orc.Spec(cfg, names, vocab, dense)
    rng = np.random.default_rng(5)
    params = orc.random_params(spec, rng)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    B, T = 8192, W.num_tasks(cfg)
    X, y = W.synth_batch(vocab, 0, B, T, seed=21)
    model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
    model.train()
    step = model.train_step_runner(B, use_graph=False)
    step.plan.X.copy_(X.to(dev()))
    step.plan.y.copy_(y.to(dev()))
    step.run()
    loss_gpu = float(step.plan.loss.item())
    opt = orc.DenseOptimizer("adam", cfg["optim_config"]["lr"])
    before = {k: v.copy() for k, v in params.items()}
    loss_ref = orc.train_step(spec, params, opt, X.numpy(), y.numpy())
    assert abs(loss_gpu - loss_ref) / loss_ref < 1e-4
    sd = {k: v.cpu().numpy() for k, v in model.state_dict().items()}
    lr = cfg["optim_config"]["lr"]
    for k, ref in params.items():
        if k.startswith("embedding_dict."):
            continue
        dv = np.abs(sd[k].astype(np.float64) - ref)
        # first Adam step moves every element by ~lr; noise-level gradients may flip sign (see test_models_gpu)
        assert dv.max() <= 2.5 * lr, k
        assert (dv > 1e-4 * max(np.abs(ref).max(), 1e-30)).mean() < 2e-3, k
    # tables: untouched rows bit-unchanged (m = v = 0 -> update 0), touched rows updated like the oracle's, the
    # outlier share counted over the touched elements (4 514 rows of the 1e7-row table at this batch)
    check_tables(vocab, names, X.numpy(), before, sd, params)
    rows = np.unique(X[:, 0].numpy().astype(np.int64))
    assert np.abs(sd["embedding_dict.c0.weight"][rows] - before["embedding_dict.c0.weight"][rows]).max() > 0.5 * lr


# ---------------------------------------------------------------------------------------------------------------
# one full-size fused step against the oracle for the other BASELINE.json configurations (the shrunken
# goldens run single-tile GEMMs; these run the persistent multi-tile paths of the real shapes)
# ---------------------------------------------------------------------------------------------------------------
_randomize = randomize_he   # (tests/conftest.py: shared with tests/golden/make_bench_losses.py)


@pytest.mark.parametrize("workload,B", [("mmoe_kuairec", 8192), ("ple_ijcai", 8192), ("star_amazon", 8192),
                                        ("pepnet_amazon", 8192)])
def test_full_size_fused_step_other_configs(W, workload, B):
    """KuaiRec-32 MMoE (E = 16, experts 512 -> 512 -> 256), Ijcai-7 PLE (2 levels), Amazon-8 STAR and PepNet at their
    full vocabularies and widths: loss, every MLP tensor and every table after one fused step (the config's own
    optimizer, dense-exact / exact-rows table update) against oracle/mmlrec_oracle.py on the same batch."""
    from oracle import mmlrec_oracle as orc
    model, cfg, vocab, dense = W.build_model(workload, dev())
    frozen = _randomize(model, 11)
    names = [f.name for f in model._sparse_cols()]
    spec = orc.Spec(cfg, names, vocab, dense)
    params = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    T = W.num_tasks(cfg)
    X, y = W.synth_batch(vocab, len(dense), B, T, seed=22)
    kind, lr = cfg["optim_config"]["optimizer"], cfg["optim_config"]["lr"]
    model.compile(kind, cfg["optim_config"]["loss"], ["auc"])
    model.train()
    step = model.train_step_runner(B, use_graph=False)
    step.plan.X.copy_(X.to(dev()))
    step.plan.y.copy_(y.to(dev()))
    step.run()
    loss_gpu = float(step.plan.loss.item())
    opt = orc.DenseOptimizer(kind, lr)
    before = {k: v.copy() for k, v in params.items()}
    loss_ref = orc.train_step(spec, params, opt, X.numpy(), y.numpy(), frozen or None)
    assert abs(loss_gpu - loss_ref) / loss_ref < 1e-4, (loss_gpu, loss_ref)
    sd = {k: v.cpu().numpy() for k, v in model.state_dict().items()}
    moved = 0
    for k, ref in params.items():
        if not k.startswith("embedding_dict."):
            dv = np.abs(sd[k].astype(np.float64) - ref)
            assert dv.max() <= 2.5 * lr, k
            assert (dv > 1e-4 * max(np.abs(ref).max(), 1e-30)).mean() < 2e-3, k
        moved += int(np.abs(ref - before[k]).max() > 0)
    assert moved >= len(params) // 2  # the step really updated the model (tables + MLP tensors)
    # tables over their touched rows only.  PepNet's scene table feeds the gates through a stop-gradient as well:
    # every table still receives its gradient through dnn_input, so all of them move.
    check_tables(vocab, names, X.numpy(), before, sd, params)


@pytest.mark.parametrize("workload,expect", [("mmoe_kuairec", "gemm_pipe_kernel"), ("ple_ijcai", "gemm"),
                                             ("star_amazon", "gemm_ws_kernel"), ("pepnet_amazon", "gemm_ws_kernel"),
                                             # AE-30 with AliExpress' 63 dense columns (K0 = 303 in rows of 304): the panel
                                             # kernel at K = 304, the narrowed input gradient under gemm_os_kernel, the
                                             # gather's dense pieces, the merged weight-gradient launch
                                             ("mmoe_ae30d", "gemm_panel_kernel")])
def test_bench_secondary_configurations_steps_match_oracle(W, workload, expect):
    """The configurations bench.py's `configs` block times, AS it times them: HIP-graph replay, the
    default stream schedule, table_update = "auto", at a batch where other code runs than at 8 192 (per-layer
    weight-gradient launches, operand magnitudes + pre-cut planes, STAR's product planes under the weight-stationary
    kernel, PepNet's 80-wide k-groups).  B = 32 768 (round 6: every large-batch path engages from 16 384 / 32 768 on -- the
    kernel-symbol assertions below hold the proof -- and the host oracle at 65 536 was most of the GPU suite's wall time on
    a 16-CPU host; the HEADLINE configuration keeps 65 536, test_bench_configuration_steps_match_oracle).
    Three steps: the first eager, the second captured and replayed, the third a pure replay.  The free-running loss
    trajectory against tests/golden/bench_losses_<workload>_he11_b32768.json (the oracle's own free run, made on the host
    by tests/golden/make_bench_losses.py); the parameters after EVERY step against ONE oracle step FROM THE MI355X'S OWN
    STATE (with He-scaled weights a free-running Adam trajectory amplifies the sign of noise-level gradients: measured
    0.4 % of a 512 x 512 weight's elements beyond 5 % of their update after two free steps at 65 536, 4 % at 8 192, with
    every step-1 element inside).  Then the kernel symbols of one more (instrumented) step."""
    import json
    import os
    from oracle import mmlrec_oracle as orc
    from mmlrec_amd import engine as E
    from conftest import GOLDEN_DIR, table_update_report
    from test_models_gpu import gpu_state
    orc.use_fast(True)
    B = 32768
    fx = json.load(open(os.path.join(GOLDEN_DIR, f"bench_losses_{workload}_he11_b{B}.json")))
    assert fx["batch"] == B and fx["workload"] == workload
    model, cfg, vocab, dense = W.build_model(workload, dev(), table_update="auto", use_hip_graph=True)
    frozen = _randomize(model, 11)
    names = [f.name for f in model._sparse_cols()]
    spec = orc.Spec(cfg, names, vocab, dense)
    T = W.num_tasks(cfg)
    kind, lr = cfg["optim_config"]["optimizer"], cfg["optim_config"]["lr"]
    model.compile(kind, cfg["optim_config"]["loss"], cfg["optim_config"]["metrics"])
    model.train()
    runner = model.train_step_runner(B, use_graph=True)   # bench.py secondary_configs' call
    skey = {"adam": ("m", "v"), "adagrad": ("sum", None), "rmsprop": ("sq", None), "sgd": (None, None)}[kind]
    for i in range(3):
        X, y = W.synth_batch(vocab, len(dense), B, T, seed=1 + i)
        sd0, mom, t = gpu_state(model)        # (lazy_exact: flushes every row first)
        runner.load(X.to(dev()), y.to(dev()))
        runner.run()
        loss_gpu = float(runner.plan.loss.item())
        loss_free = fx["loss_sum_per_step"][i]
        assert abs(loss_gpu - loss_free) / loss_free < 1e-4, (i, loss_gpu, loss_free)
        # the oracle's step from exactly where the MI355X stood
        params = {k: v.copy() for k, v in sd0.items() if not k.endswith("num_batches_tracked")}
        opt = orc.DenseOptimizer(kind, lr)
        opt.t = t
        for k, (s1, s2) in mom.items():
            st = {}
            if skey[0] and s1 is not None:
                st[skey[0]] = s1.copy()
            if skey[1] and s2 is not None:
                st[skey[1]] = s2.copy()
            if st:
                opt.state[k] = st
        loss_ref = orc.train_step(spec, params, opt, X.numpy(), y.numpy(), frozen or None)
        assert abs(loss_gpu - loss_ref) / loss_ref < 1e-4, (i, loss_gpu, loss_ref)
        sd = {k: v.cpu().numpy() for k, v in model.state_dict().items()}
        moved = 0
        for k, ref in params.items():
            if k.startswith("embedding_dict."):
                continue
            dv = np.abs(sd[k].astype(np.float64) - ref)
            assert dv.max() <= (25.0 if kind == "rmsprop" else 2.5) * lr, (i, k)
            # He-scaled weights at this batch: the two sides' pre-activations differ by ~3e-7 of their scale, so of the
            # 65 536 x ~2 000 first-layer ReLUs ~100 sit on different sides of zero; each flip changes one row of that
            # layer's weight gradient by one sample's term, ~0.5 % of the row's typical element, i.e. > 5 % for the
            # row's smallest elements -- measured 0.3-0.4 % of a tensor's elements outside 5 % of their Adam update
            # (PLE 0.31 %, PepNet 0.37 %; the AE-30 test above starts from the reference's 1e-4-scale weights and stays
            # at 0.03 %).  A wrong tile or a stale operand moves far more than 1 %.
            check_update(k, sd0[k], sd[k], ref, allow=1e-2)
            moved += int(np.abs(ref - sd0[k]).max() > 0)
        assert moved >= 4
        # tables: rows without optimizer state that this batch does not touch stay bit-identical; every row that moved on
        # either side is compared element-wise (rows of earlier batches keep moving under dense Adam semantics)
        for f, v in enumerate(vocab):
            k = f"embedding_dict.{names[f]}.weight"
            b, a, r = sd0[k], sd[k], params[k]
            rows = np.nonzero(np.abs(r - b).max(1) + np.abs(a - b).max(1))[0]
            touched = np.unique(X[:, f].numpy().astype(np.int64))
            assert np.isin(touched, rows).mean() > 0.99, k        # the batch's rows moved
            share, rel = table_update_report(b, a, r, rows)
            # (5e-3: soaked in round 6 -- 36 fresh-process runs gave 0.0025-0.003 on KuaiRec-32's 62- and 199-row tables at
            # the third free-running Adam step in 3 of them, elements whose gradient sits at the scatter's summation-order
            # noise; the MLP tensors above keep their 1e-2 / 2e-3 bounds, a wrong row or a stale buffer moves whole rows)
            assert share < 5e-3, (i, k, share, rel, len(rows))
    segs = [runner.whole] if runner.whole is not None else [runner.front, runner.tail, runner.sideq]
    assert sum(s_.n_graphs for s_ in segs if s_ is not None) >= 1   # the replayed path really ran
    # which kernels this configuration's step launches at this size
    p = runner.plan
    acc = {}
    E.Plan.run_timed(list(p.fwd) + list(p.head_train) + list(p.bwd) + list(p.bwd_tail) + list(p.head_side) +
                     list(p.bwd_side), acc)
    assert any(expect in k for k in acc), sorted(acc)
    if workload == "mmoe_ae30d":
        assert any("gemm_os_kernel" in k for k in acc) and any("gemm_nt_kernel" in k for k in acc), sorted(acc)
    gemms = [k for k in acc if k.startswith("gemm")]
    # two scaled fp16 planes (operand magnitudes on from 32 768 samples): no launch falls back to the bf16 x 3 form
    assert gemms and not any(k.startswith("gemm_pipe_kernel") and ", 3, " in k for k in gemms), gemms


# ---------------------------------------------------------------------------------------------------------------
# The BENCHMARKED configuration itself (every full-size step above runs B = 8 192 eagerly; bench.py times
# B = 65 536, HIP-graph replay, two streams, the > 8 192 code paths: per-layer weight-gradient launches, the single
# input-gradient GEMM, opt_dense_kernel<true> beside the weight-gradient stream, marked-gradient reads)
# ---------------------------------------------------------------------------------------------------------------
_BENCH_ORACLE = {}


def _bench_oracle(W, cfg, names, vocab, dense, start, nsteps=3):
    """The ORACLE's trajectory over bench.py's first `nsteps` batches (B = 65 536, seeds 1, 2, 3) from the reference's
    seed-0 initialisation under dense Adam -- computed ONCE per pytest process and shared by the five tests that run this
    same sequence on the MI355X under different schedules (one stream / two streams / lazy_exact / row-sharded dense /
    row-sharded lazy): every one of them starts from the same parameters (checked: `start` must equal the cached start bit
    for bit) and must arrive at the same dense-Adam state.  Returns (per-step losses, final parameters, batches X)."""
    from oracle import mmlrec_oracle as orc
    orc.use_fast(True)
    c = _BENCH_ORACLE.get("traj")
    if c is None:
        spec = orc.Spec(cfg, names, vocab, dense)
        params = {k: v.copy() for k, v in start.items()}
        opt = orc.DenseOptimizer("adam", cfg["optim_config"]["lr"])
        B, T = 65536, W.num_tasks(cfg)
        losses, Xs = [], []
        for i in range(nsteps):
            X, y = W.synth_batch(vocab, 0, B, T, seed=1 + i)
            Xs.append(X.numpy())
            losses.append(orc.train_step(spec, params, opt, X.numpy(), y.numpy()))
        c = _BENCH_ORACLE["traj"] = dict(start={k: v.copy() for k, v in start.items()}, losses=losses, params=params, Xs=Xs)
    assert set(c["start"]) == set(start) and all(np.array_equal(c["start"][k], start[k]) for k in start), \
        "the shared oracle trajectory was computed from another initial state"
    return c["losses"], c["params"], c["Xs"]


def _bench_model(W, table_update, scatter_mode=None):
    """What bench.py builds: mmoe_ae30, reference initialisation (seed 0, built on the host), HIP graphs on.  The library's
    default scatter (float atomics, what fit() trains with) unless `scatter_mode` says otherwise; bench.py times one GPU
    with scatter_mode="deterministic" (bitwise repeatable runs)."""
    kw = {} if scatter_mode is None else dict(scatter_mode=scatter_mode)
    model, cfg, vocab, dense = W.build_model("mmoe_ae30", dev(), table_update=table_update, use_hip_graph=True, **kw)
    model.compile(cfg["optim_config"]["optimizer"], cfg["optim_config"]["loss"], cfg["optim_config"]["metrics"])
    model.train()
    return model, cfg, vocab, dense


@pytest.mark.parametrize("table_update,streams", [("dense_exact", 1), ("lazy_exact", 1), ("dense_exact", 2)])
def test_bench_configuration_steps_match_oracle(W, table_update, streams):
    """bench.py's step -- B = 65 536, use_graph=True, one stream (the default since round 5: the whole step ONE HIP graph)
    or the forked two-stream tail (--streams 2), default dense-update schedule --
    for THREE steps on bench.py's batches (seeds 1, 2, 3): step 0 runs eagerly, step 1 captures the HIP graphs and
    replays them, step 2 is a pure replay.  Losses, every MLP tensor and every table (touched rows element-wise,
    untouched rows bit for bit) against oracle.train_step on the same batches.  lazy_exact: after the flush that
    state_dict() triggers, the same dense-Adam state."""
    _check_bench_steps(W, table_update, streams, None)


def test_bench_deterministic_scatter_steps_match_oracle(W):
    """The step a one-GPU bench.py run times: as test_bench_configuration_steps_match_oracle (B = 65 536, one stream,
    eager step, capture, replay; losses, MLP tensors, every table against the oracle) with the deterministic
    table-gradient scatter (integer fixed-point row totals + the finalize launch) -- and that path really taken."""
    _check_bench_steps(W, "dense_exact", 1, "deterministic")


def _check_bench_steps(W, table_update, streams, scatter_mode):
    model, cfg, vocab, dense = _bench_model(W, table_update, scatter_mode)
    names = [f.name for f in model._sparse_cols()]
    before = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    B, T, lr = 65536, W.num_tasks(cfg), cfg["optim_config"]["lr"]
    nsteps = 3
    losses_ref, params, Xs = _bench_oracle(W, cfg, names, vocab, dense, before, nsteps)
    runner = model.train_step_runner(B, use_graph=True, overlap=(streams == 2), split_dense=False)  # bench.py's call
    assert runner.use_graph and runner.overlap == (streams == 2) and (runner.whole is not None) == (streams == 1)
    if streams == 1:
        # round 6: the top of the network (last tower layer + heads + BCE + the towers' input gradient) is ONE launch of
        # the one-stream step (csrc/tower_head.hip; passes.fuse_tower_head) -- and the three launches it replaces are gone
        from mmlrec_amd import _lib
        lib_ = _lib.load()
        calls = [c for part in runner.whole.parts if part[0] == "c" for c in part[1]]
        assert runner.tower_head_fused and sum(c[0] is lib_.mml_tower_head_fwd_bwd for c in calls) == 1
        assert not any(c[0] is lib_.mml_head_bce_fwd_bwd_phase for c in calls)
        det = sum(c[0] is lib_.mml_scatter_bwd_det for c in calls)
        assert det == (1 if scatter_mode == "deterministic" else 0), det
    for i in range(nsteps):
        X, y = W.synth_batch(vocab, 0, B, T, seed=1 + i)
        runner.plan.X.copy_(X.to(dev()))
        runner.plan.y.copy_(y.to(dev()))
        runner.run()
        loss_gpu = float(runner.plan.loss.item())
        assert abs(loss_gpu - losses_ref[i]) / losses_ref[i] < 1e-4, (i, loss_gpu, losses_ref[i])
    if runner.whole is None:
        assert runner.front.n_graphs >= 1 and runner.tail.n_graphs >= 1  # the replayed path really ran
    else:
        assert runner.whole.n_graphs >= 1
    sd = {k: v.cpu().numpy() for k, v in model.state_dict().items()}  # (lazy_exact: flushes every row first)
    # From the reference's 1e-4-scale initialisation the first-layer weight gradients sit at Adam's eps (1e-8), where the
    # update lr g / (|g| + eps) amplifies the fp32 summation-order noise of a 65 536-term sum (the oracle's own numpy sum
    # carries the same noise): a max-normalised 1e-4 bound is not attainable there, the element-wise UPDATE criterion
    # (5 % of the reference update, outliers < 0.2 %; measured: <= 0.03 % beyond 5 %) is -- for MLP tensors and tables
    # alike.  Gross errors (a stale buffer in a replayed graph, a race between the two streams) move elements by ~lr.
    for k, ref in params.items():
        if k.startswith("embedding_dict."):
            continue
        dv = np.abs(sd[k].astype(np.float64) - ref)
        assert dv.max() <= 2.5 * lr * nsteps, k
        check_update(k, before[k], sd[k], ref)
    check_tables(vocab, names, np.concatenate(Xs), before, sd, params)


@pytest.mark.parametrize("table_update", ["dense_exact", "lazy_exact"])
def test_row_sharded_bench_configuration_steps_match_oracle(W, table_update):
    """The row-sharded step at the benchmark's configuration (only a builder-side MMLREC_BENCH_FORCE_SHARD run
    covered it): B = 65 536, 1-rank RCCL group, de-duplicated exchange, HIP-graph segments, and the routing of batch
    k + 1 prefetched on the side stream while step k is in flight (bench.py's loop: run(); prefetch(next)).  Three steps
    on bench.py's batches against oracle.train_step -- losses, every MLP tensor, every table row the batches touched
    element-wise and every other row bit for bit after the shards are gathered back (state_dict())."""
    import os
    import torch.distributed as dist
    from mmlrec_amd import parallel
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        created = True
    try:
        model, cfg, vocab, dense = _bench_model(W, table_update)
        names = [f.name for f in model._sparse_cols()]
        before = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
        B, T, lr = 65536, W.num_tasks(cfg), cfg["optim_config"]["lr"]
        nsteps = 3
        losses_ref, params, Xs = _bench_oracle(W, cfg, names, vocab, dense, before, nsteps)
        par = parallel.shard_model(model, dist, B, mode="row_sharded")
        runner = model.train_step_runner(B, use_graph=True, split_dense=False)   # (bench.py's default schedule)
        batches = [W.synth_batch(vocab, 0, B, T, seed=1 + i) for i in range(nsteps)]
        dbatches = [(x.to(dev()), y.to(dev())) for x, y in batches]
        for i in range(nsteps):
            if not runner._has_next:          # (step 0 routes its batch itself; the others were prefetched)
                runner.load(*dbatches[i])
            else:
                assert i > 0
            runner.run()
            if i + 1 < nsteps:
                runner.prefetch(*dbatches[i + 1])
            loss_gpu = float(runner.plan.loss.item())
            assert abs(loss_gpu - losses_ref[i]) / losses_ref[i] < 1e-4, (i, loss_gpu, losses_ref[i])
        runner.drop_prefetch()
        segs = [runner.whole] if runner.whole is not None else [runner.front, runner.sideq, runner.tail]
        assert sum(s_.n_graphs for s_ in segs) >= 2  # the runs of launches between the collectives were captured
        assert par.dirty
        sd = {k: v.cpu().numpy() for k, v in model.state_dict().items()}  # gathers the shards (and flushes lazy rows)
        assert not par.dirty
        for k, ref in params.items():
            if k.startswith("embedding_dict."):
                continue
            dv = np.abs(sd[k].astype(np.float64) - ref)
            assert dv.max() <= 2.5 * lr * nsteps, k
            check_update(k, before[k], sd[k], ref)
        check_tables(vocab, names, np.concatenate(Xs), before, sd, params)
    finally:
        if created:
            torch.cuda.synchronize()
            dist.destroy_process_group()


def test_bench_sequence_losses_match_fixture(W):
    """The loss trajectory bench.py reports: its exact step sequence (4 resident batches, seeds 1-4, rotated) for 25
    steps (the driver's --warmup 5 --steps 20) against tests/golden/bench_losses_mmoe_ae30.json, which the ORACLE
    produced on the host (tests/golden/make_bench_losses.py).  bench.py checks itself against the same file."""
    import json
    import os
    from conftest import GOLDEN_DIR
    fx = json.load(open(os.path.join(GOLDEN_DIR, "bench_losses_mmoe_ae30.json")))
    want = fx["loss_sum_per_step"]
    model, cfg, vocab, dense = _bench_model(W, "dense_exact")
    B, T = fx["batch"], W.num_tasks(cfg)
    batches = [W.synth_batch(vocab, 0, B, T, seed=1 + i) for i in range(4)]
    batches = [(x.to(dev()), y.to(dev())) for x, y in batches]
    runner = model.train_step_runner(B, use_graph=True, split_dense=False)   # (bench.py's default schedule)
    from bench import loss_tolerance
    worst = []
    for i in range(25):
        X, y = batches[i % 4]
        runner.plan.X.copy_(X)
        runner.plan.y.copy_(y)
        runner.run()
        got = float(runner.plan.loss.item())
        rel = abs(got - want[i]) / want[i]
        worst.append(rel)
        assert rel < loss_tolerance(i), (i, got, want[i], rel)
    print("bench-sequence loss rel. errors:", ["%.1e" % r for r in worst])


@pytest.mark.parametrize("storage", ["bf16", "fp32"])
def test_bf16_operand_mode_full_size_kuairec(W, storage, monkeypatch):
    """BASELINE configs[1] names bf16: the opt-in GEMM mode 1 (operands rounded to bf16, fp32 accumulate) -- with the
    activations and gradients between GEMMs STORED as bf16 and every layer group on csrc/gemm16.hip (round 5, the default
    of mode 1), or with fp32 buffers and the operands rounded in registers (MMLREC_BF16_STORAGE=0): the same products,
    so the same tolerances -- on the FULL KuaiRec-32 shapes (E = 16, experts 512 -> 512 -> 256) at B = 8 192 against the
    fp32 oracle: loss within 2e-3 (measured 3e-6), every MLP weight gradient within 6 % relative rms (the shrunken golden
    with 64 samples only supported 15 %), table gradients within 10 % relative rms over the touched rows.  The reference
    has no bf16 path; SURVEY 8 (A5) probed rms(dlogit)/rms(logit) ~ 8e-3 for it under CPU autocast(bfloat16)."""
    from oracle import mmlrec_oracle as orc
    from mmlrec_amd import _lib
    lib = _lib.load()
    mode0 = lib.mml_gemm_get_mode()
    monkeypatch.setenv("MMLREC_BF16_STORAGE", "1" if storage == "bf16" else "0")
    try:
        lib.mml_gemm_set_mode(1)
        model, cfg, vocab, dense = W.build_model("mmoe_kuairec", dev())
        _randomize(model, 11)
        names = [f.name for f in model._sparse_cols()]
        spec = orc.Spec(cfg, names, vocab, dense)
        params = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
        B, T = 8192, W.num_tasks(cfg)
        X, y = W.synth_batch(vocab, len(dense), B, T, seed=23)
        model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
        model.train()
        step = model.train_step_runner(B, use_graph=False)
        step.plan.X.copy_(X.to(dev()))
        step.plan.y.copy_(y.to(dev()))
        step.plan.run_train_fwd_bwd()  # forward + BCE + backward, no optimizer: the gradients stay in their buffers
        torch.cuda.synchronize()
        calls = list(step.plan.fwd) + list(step.plan.bwd) + list(step.plan.bwd_side)
        n16 = sum(c[0] in (lib.mml_g16_tn, lib.mml_g16_wgrad) for c in calls)
        n32 = sum(c[0] in (lib.mml_gemm_grouped_fwd, lib.mml_gemm_grouped_dgrad, lib.mml_gemm_grouped_wgrad_phase)
                  for c in calls)
        if storage == "bf16":
            # every layer group of the model (first / second expert layers, gate networks, towers; forward, input and
            # weight gradients) runs the bf16-storage kernels, the gather writes bf16, the row kernels bf16 gradients
            assert n16 >= 9 and n32 == 0, (n16, n32)
            assert any(c[0] is lib.mml_gather16_fwd for c in calls)
            assert step.plan.layer_outputs["dnn_input"].buf.dtype == torch.bfloat16
            assert lib.mml_g16_last_kernel().decode().startswith("g16_")
        else:
            assert n16 == 0 and n32 >= 6, (n16, n32)
            assert ", 1, " in lib.mml_gemm_last_kernel().decode()  # the one-plane bf16 kernel really ran
        loss_ref, grads, _ = orc.loss_and_grads(spec, params, X.numpy(), y.numpy())
        loss_gpu = float(step.plan.loss.item())
        assert abs(loss_gpu - loss_ref) / loss_ref < 2e-3, (loss_gpu, loss_ref)
        st = model._store()
        worst = {}
        for k, gr in grads.items():
            got = st.pvals[k].grad.cpu().numpy().astype(np.float64)
            if k.startswith("embedding_dict."):
                f = names.index(k.split(".")[1])
                rows = np.unique(X[:, f].numpy().astype(np.int64))
                got, gr = got[rows], gr[rows]
            rms = np.sqrt(np.mean((got - gr) ** 2)) / max(np.sqrt(np.mean(gr.astype(np.float64) ** 2)), 1e-30)
            # the table gradients come out of THREE chained reduced-precision input-gradient GEMMs and are sums with
            # cancellation over the samples of a row: 10 % there (measured 7.7 %), 6 % for every MLP tensor (measured 5.0 %)
            lim = 0.10 if k.startswith("embedding_dict.") else 0.06
            worst[lim] = max(worst.get(lim, 0.0), rms)
            assert rms < lim, (k, rms)
        print("bf16 operand mode, full-size KuaiRec-32: loss rel err %.2e, worst gradient relative rms %s"
              % (abs(loss_gpu - loss_ref) / loss_ref, {("tables" if a > 0.06 else "mlp"): round(float(b), 4) for a, b in worst.items()}))
    finally:
        lib.mml_gemm_set_mode(mode0)


# ---------------------------------------------------------------------------------------------------------------
# BASELINE configs[1] AS bench.py TIMES IT: bf16 storage, HIP-graph replay WITH the optimizer, the
# merged bf16 weight-gradient launches, the per-step re-cast of the bf16 weight copies -- a stale copy in a replayed graph is
# what nothing else would catch
# ---------------------------------------------------------------------------------------------------------------
_BF16_ORACLE = {}


@pytest.mark.parametrize("inner_fork", ["default", "0"])
def test_bf16_bench_configuration_steps_match_oracle(W, inner_fork, monkeypatch):
    """bench.py's `configs[1] ... bf16` entry: mmoe_kuairec under GEMM mode 1 with bf16 storage, table_update "auto",
    train_step_runner(B, use_graph=True) -- step 0 eager, step 1 captured + replayed, step 2 a pure replay -- at B = 32 768
    (every large-batch path of the bf16 family engages from 16 384 on; asserted below) against the fp32 ORACLE's free-running
    trajectory from the same He-scaled start (computed once, shared by the two schedules): per-step loss within 2e-3 (the
    tolerance of test_bf16_operand_mode_full_size_kuairec), the total update of every MLP tensor and of every table's
    touched rows within a relative rms bound, and after EVERY step each bf16 weight copy of the plan (plan.cast16_items)
    equal to the bf16 rounding of the fp32 master weight THAT STEP STARTED FROM -- while the master weights moved, i.e. the
    replayed graph re-casts them.  inner_fork "default": the weight-gradient launches on the second branch of the step's
    graph (on from 16 384 samples; soaked in round 6); "0": the one-branch graph (MMLREC_INNER_FORK=0)."""
    from oracle import mmlrec_oracle as orc
    from mmlrec_amd import _lib
    from mmlrec_amd import engine as E
    orc.use_fast(True)
    lib = _lib.load()
    mode0 = lib.mml_gemm_get_mode()
    monkeypatch.setenv("MMLREC_BF16_STORAGE", "1")
    if inner_fork == "default":
        monkeypatch.delenv("MMLREC_INNER_FORK", raising=False)
    else:
        monkeypatch.setenv("MMLREC_INNER_FORK", inner_fork)
    B, nsteps = 32768, 3
    try:
        lib.mml_gemm_set_mode(1)
        model, cfg, vocab, dense = W.build_model("mmoe_kuairec", dev(), table_update="auto", use_hip_graph=True)
        _randomize(model, 11)
        names = [f.name for f in model._sparse_cols()]
        T = W.num_tasks(cfg)
        kind, lr = cfg["optim_config"]["optimizer"], cfg["optim_config"]["lr"]
        model.compile(kind, cfg["optim_config"]["loss"], cfg["optim_config"]["metrics"])
        model.train()
        before = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
        batches = [W.synth_batch(vocab, len(dense), B, T, seed=1 + i) for i in range(nsteps)]
        if "traj" not in _BF16_ORACLE:   # the fp32 oracle's free run (host): once for both schedules
            spec = orc.Spec(cfg, names, vocab, dense)
            params = {k: v.copy() for k, v in before.items()}
            opt = orc.DenseOptimizer(kind, lr)
            losses = [orc.train_step(spec, params, opt, X.numpy(), y.numpy()) for X, y in batches]
            _BF16_ORACLE["traj"] = (losses, params, {k: v.copy() for k, v in before.items()})
        losses_ref, params_ref, start_ref = _BF16_ORACLE["traj"]
        assert all(np.array_equal(start_ref[k], before[k]) for k in before)
        runner = model.train_step_runner(B, use_graph=True)   # bench.py secondary_configs' call
        p = runner.plan
        # what bench.py's run launches: every layer group on the bf16-storage kernels, the weight gradients merged
        calls = [c for part in runner.whole.parts if part[0] == "c" for c in part[1]]
        forked = getattr(runner, "inner_fork", None)
        if forked is not None:
            calls += list(forked.calls)
        assert (forked is not None) == (inner_fork == "default")   # (on from 16 384 samples by default)
        n16 = sum(c[0] in (lib.mml_g16_tn, lib.mml_g16_wgrad) for c in calls if c[0] is not E.INLINE)
        n32 = sum(c[0] in (lib.mml_gemm_grouped_fwd, lib.mml_gemm_grouped_dgrad, lib.mml_gemm_grouped_wgrad_phase)
                  for c in calls if c[0] is not E.INLINE)
        assert n16 >= 9 and n32 == 0, (n16, n32)
        merged = [c for c in calls if c[0] is lib.mml_g16_wgrad and c[1][4] == 1 and "problems)" in c[2]["kernel"]]
        assert merged and any(c[1][1] >= 2 for c in merged), [c[2]["kernel"] for c in calls if c[0] is lib.mml_g16_wgrad]
        fns = [c[0] for c in calls]
        assert p.cast16_items and lib.mml_cast16_batch in fns and \
            fns.index(lib.mml_cast16_batch) < fns.index(lib.mml_g16_tn)   # the re-cast opens the step (inside the graph)
        assert p.layer_outputs["dnn_input"].buf.dtype == torch.bfloat16
        changed = 0
        for i, (X, y) in enumerate(batches):
            w_start = [w.detach().clone() for w, _, _ in p.cast16_items]
            c_prev = [dst.clone() for _, dst, _ in p.cast16_items]
            runner.load(X.to(dev()), y.to(dev()))
            runner.run()
            loss_gpu = float(p.loss.item())
            assert abs(loss_gpu - losses_ref[i]) / losses_ref[i] < 2e-3, (i, loss_gpu, losses_ref[i])
            for (w, dst, tr), w0, c0 in zip(p.cast16_items, w_start, c_prev):
                want = (w0.t() if tr else w0).to(torch.bfloat16)
                assert torch.equal(dst.view(torch.int16), want.contiguous().view(torch.int16)), (i, tuple(w.shape), tr)
                assert not torch.equal(w, w0)                       # the master weight moved in this step ...
                if i > 0:
                    changed += int(not torch.equal(dst, c0))        # ... and its copy followed it in the next
        assert changed == 2 * len(p.cast16_items)                   # (steps 1 and 2: the captured graph and its replay)
        assert runner.whole.n_graphs >= 1
        assert lib.mml_g16_last_kernel().decode().startswith("g16_")
        sd = {k: v.cpu().numpy() for k, v in model.state_dict().items()}
        worst = {}
        for k, ref in params_ref.items():
            b, a = before[k].astype(np.float64), sd[k].astype(np.float64)
            d_ref, d_got = ref.astype(np.float64) - b, a - b
            if k.startswith("embedding_dict."):
                f = names.index(k.split(".")[1])
                rows = np.unique(np.concatenate([X[:, f].numpy().astype(np.int64) for X, _ in batches]))
                d_ref, d_got = d_ref[rows], d_got[rows]
            rms = np.sqrt(np.mean((d_got - d_ref) ** 2)) / max(np.sqrt(np.mean(d_ref ** 2)), 1e-30)
            kind_k = "tables" if k.startswith("embedding_dict.") else ("weights" if ref.ndim == 2 else "biases")
            worst[kind_k] = max(worst.get(kind_k, (0.0, ""))[0], float(rms)), k
            assert np.abs(d_got).max() <= 2.5 * lr * nsteps, k
        print("bf16 bench configuration (B = %d, graph replay, fork %s): worst relative rms of the 3-step update %s"
              % (B, inner_fork, {k: (round(v[0], 4), v[1]) for k, v in worst.items()}))
        # three free-running Adam steps whose gradients carry bf16 rounding (5 % relative rms per MLP tensor, 8 % per table
        # at B = 8 192: the test above): the UPDATE lr m / (sqrt(v) + eps) follows the gradient's direction, so the same
        # order of deviation, plus the sign flips of gradients that sit at the noise level -- a bias gradient is the column
        # sum of 32 768 bf16-stored gradient rows, the few elements of it near zero flip under Adam's normalisation
        # (measured: weights 0.32 -- the [1, 128] tower output rows --, biases 0.30, tables 0.33; a stale operand or a wrong
        # tile gives >= 1, and the bf16 copies themselves are checked bit for bit above)
        for kind_k, lim in (("weights", 0.5), ("biases", 0.5), ("tables", 0.5)):
            assert worst.get(kind_k, (0.0, ""))[0] < lim, (kind_k, worst[kind_k])
    finally:
        lib.mml_gemm_set_mode(mode0)
