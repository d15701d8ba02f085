"""Models of the zoo with multi-valued (pooled) feature columns, through BaseModel, engine.PooledGatherOp and the fused
train step.

No fixture made from the reference backs this file yet (tests/golden/make_golden_pooled.py is not written), so nothing
here compares with the reference's own numbers.  What stands in, and why it is independent of the code under test:

  * a pooled feature of maxlen 1 pooled by `sum` whose ids are never 0 computes exactly what a single-valued feature
    computes.  Two models with the SAME state, one declaring the column as a SparseFeat (the path the reference-made
    fixtures of tests/test_models_gpu.py pin), one as a VarLenSparseFeat, must agree in dnn_input (bits), predictions,
    loss, gradients and fused steps of every optimizer / table_update mode, graph off and on;
  * dnn_input of a full pooled schema (mean / length mode on a table shared with an id column, max / mask, sum / mask)
    against the float64 restatement of tests/test_pooled_functional_gpu.py, with its worst-case fp32 bounds;
  * the three table_update modes against each other from the same state (the arbiter the issue names: touched rows by
    the update criterion of conftest.table_update_report at share < 2e-3, rows no batch touched np.array_equal between
    dense_exact and flushed lazy_exact);
  * the refusals, and that a model without pooled columns still records today's gather and scatter calls.
"""
import copy
import json

import numpy as np
import pytest
import torch

from conftest import load_golden, table_update_report
from test_pooled_functional_gpu import elem_rel, make_x, reference64, rel, schema

pytestmark = pytest.mark.gpu

RTOL = 1e-4


def config(name="mmoe_kuairec", emb=8, **model_kw):
    cfg = json.loads(str(load_golden(name)["cfg"]))
    cfg["model_config"]["emb"] = emb
    cfg["model_config"].update(model_kw)
    return cfg


def make_model(cls_name, cols, cfg, seed=0):
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import model as M
    torch.manual_seed(seed)
    return getattr(M, cls_name)(cols, device="cuda:0", config=cfg)


def pair_columns(E, pooled):
    from mmlrec_amd.model import DenseFeat, SparseFeat, VarLenSparseFeat
    item = SparseFeat("item", 200, embedding_dim=E)
    return [SparseFeat("user", 50, embedding_dim=E),
            VarLenSparseFeat(item, maxlen=1, combiner="sum") if pooled else item,
            DenseFeat("price", 1)]


def pair_batch(B, seed):
    rng = np.random.default_rng(seed)
    X = np.zeros((B, 3), np.float32)
    X[:, 0] = rng.integers(0, 50, B)
    X[:, 1] = np.minimum(rng.zipf(1.3, B), 199)  # never 0: every position valid
    X[:, 2] = rng.standard_normal(B)
    y = (rng.random((B, 2)) < 0.4).astype(np.float32)
    return X, y


def run_steps(model, kind, cfg, batches, graph):
    model.compile(kind, cfg["optim_config"]["loss"], ["auc"])
    model.train()
    losses = []
    for X, y in batches:
        step = model.train_step_runner(X.shape[0], use_graph=graph)
        step.plan.X.copy_(torch.from_numpy(X).cuda())
        step.plan.y.copy_(torch.from_numpy(y).cuda())
        step.run()
        losses.append(float(step.plan.loss.item()))
    return losses, {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("E", [8, 16])
def test_maxlen1_sum_model_equals_the_single_valued_model(E):
    cfg = config(emb=E)
    a = make_model("MMOE", pair_columns(E, False), cfg)
    b = make_model("MMOE", pair_columns(E, True), cfg)
    assert set(a.state_dict()) == set(b.state_dict())
    b.load_state_dict(a.state_dict())
    X, y = pair_batch(64, 1)
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    outs = []
    for m in (a, b):
        m.eval()
        m.update_save(True)
        with torch.no_grad():
            yp = m(Xd)
        outs.append((yp.cpu().numpy(), m.layer_output_dict["dnn_input"].cpu().numpy()))
    assert np.array_equal(outs[0][1], outs[1][1])  # the same rows, copied
    assert np.array_equal(outs[0][0], outs[1][0])
    grads = []
    for m in (a, b):
        m.train()
        loss = torch.nn.functional.binary_cross_entropy(m(Xd), yd, reduction="sum")
        loss.backward()
        grads.append((float(loss), {n: p.grad.cpu().numpy() for n, p in m.named_parameters() if p.grad is not None}))
    assert abs(grads[0][0] - grads[1][0]) <= RTOL * abs(grads[0][0])
    assert set(grads[0][1]) == set(grads[1][1])
    for n, g in grads[0][1].items():
        assert rel(grads[1][1][n], g) < RTOL, n
        if n.startswith("embedding_dict."):
            assert elem_rel(grads[1][1][n], g) <= 1.0, n


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("kind,tu", [("adam", "dense_exact"), ("adam", "lazy_exact"), ("adagrad", "sparse_rows"),
                                     ("rmsprop", "dense_exact"), ("sgd", "sparse_rows")])
def test_maxlen1_fused_steps_equal_the_single_valued_model(kind, tu, graph):
    E = 8
    cfg = config(emb=E, table_update=tu)
    a = make_model("MMOE", pair_columns(E, False), cfg)
    b = make_model("MMOE", pair_columns(E, True), cfg)
    b.load_state_dict(a.state_dict())
    before = {k: v.detach().cpu().numpy().copy() for k, v in a.state_dict().items()}
    batches = [pair_batch(64, s) for s in (1, 2, 3)]
    la, sa = run_steps(a, kind, cfg, batches, graph)
    lb, sb = run_steps(b, kind, cfg, batches, graph)
    assert b.optimizer().table_update == a.optimizer().table_update
    assert np.allclose(lb, la, rtol=RTOL), (la, lb)
    lr = cfg["optim_config"]["lr"]
    for k in sa:
        if k.startswith("embedding_dict."):
            col = 0 if ".user." in k else 1
            rows = np.unique(np.concatenate([X[:, col] for X, _ in batches]).astype(np.int64))
            idle = np.ones(sa[k].shape[0], bool)
            idle[rows] = False
            assert np.array_equal(sb[k][idle], sa[k][idle]), k
        else:
            rows = np.arange(before[k].shape[0]) if before[k].ndim else np.arange(1)
        b0 = before[k] if before[k].ndim else before[k].reshape(1)
        share, r = table_update_report(b0, sb[k].reshape(b0.shape), sa[k].reshape(b0.shape), rows)
        assert share < 2e-3, (k, share, r)
        assert np.abs(sb[k].astype(np.float64) - sa[k]).max() <= 2.5 * lr * 3, k


def full_model(E, cls="MMOE", tu="dense_exact", cfg_name="mmoe_kuairec"):
    from mmlrec_amd.model.utils import build_input_features
    cols = schema(E)
    cfg = config(cfg_name, emb=E, table_update=tu)
    return make_model(cls, cols, cfg), cfg, cols, build_input_features(cols)


@pytest.mark.parametrize("cls,cfg_name", [("MMOE", "mmoe_kuairec"), ("SharedBottom", "sharedbottom_ml")])
@pytest.mark.parametrize("E", [8, 16])
def test_pooled_schema_state_forward_and_dnn_input(cls, cfg_name, E):
    model, cfg, cols, fi = full_model(E, cls, cfg_name=cfg_name)
    sd = model.state_dict()
    tabs = sorted(k for k in sd if k.startswith("embedding_dict."))
    assert tabs == [f"embedding_dict.{n}.weight" for n in ("cats", "item", "tags", "user")]  # hist shares item's table
    assert tuple(sd["embedding_dict.item.weight"].shape) == (500, E)
    assert model.compute_input_dim(cols) == 5 * E + 1
    with torch.no_grad():
        for k in tabs:
            sd[k].copy_(torch.randn_like(sd[k]) * 0.1)
    X = make_x(cols, fi, 64, np.random.default_rng(3))
    model.eval()
    model.update_save(True)
    with torch.no_grad():
        y = model(torch.from_numpy(X).cuda())
    assert y.shape == (64, 2) and bool(torch.isfinite(y).all())
    got = model.layer_output_dict["dnn_input"].cpu().numpy()
    t64 = {k.split(".")[1]: sd[k].detach().cpu().double() for k in tabs}
    ref, bound = reference64(cols, fi, t64, X)
    exact = (bound == 0).numpy()
    assert got.shape == tuple(ref.shape)
    assert np.array_equal(got[exact], ref.numpy().astype(np.float32)[exact])
    assert np.all(np.abs(got.astype(np.float64) - ref.numpy()) <= bound.numpy())
    # predict after a state_dict round trip and a deepcopy returns the same bits
    twin, _, _, _ = full_model(E, cls, cfg_name=cfg_name)
    twin.load_state_dict(model.state_dict())
    twin.eval()
    clone = copy.deepcopy(model)
    with torch.no_grad():
        assert torch.equal(twin(torch.from_numpy(X).cuda()), y)
        assert torch.equal(clone(torch.from_numpy(X).cuda()), y)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("kind", ["adam", "adagrad"])
def test_table_update_modes_agree_from_the_same_state(kind, graph):
    """dense_exact, sparse_rows and lazy_exact from one state over three batches.  Adagrad (and SGD) do not move a row
    with a zero gradient, so all three modes are the same update; Adam's sparse_rows is a different optimizer on rows a
    batch skips, so it is compared after ONE step only."""
    E = 8
    ref_model, cfg, cols, fi = full_model(E, tu="dense_exact")
    with torch.no_grad():
        for n, p in ref_model.named_parameters():
            if n.startswith("embedding_dict."):
                p.copy_(torch.randn_like(p) * 0.1)
    state = {k: v.clone() for k, v in ref_model.state_dict().items()}
    before = {k: v.cpu().numpy().copy() for k, v in state.items()}
    rng = np.random.default_rng(9)
    batches = [(make_x(cols, fi, 64, rng), (rng.random((64, 2)) < 0.4).astype(np.float32)) for _ in range(3)]
    results = {}
    for tu in ("dense_exact", "lazy_exact", "sparse_rows"):
        m, c, _, _ = full_model(E, tu=tu)
        m.load_state_dict(state)
        n_steps = 1 if (kind == "adam" and tu == "sparse_rows") else 3
        results[tu] = run_steps(m, kind, c, batches[:n_steps], graph) + (n_steps,)
    dense_l, dense_s, _ = results["dense_exact"]
    dense1 = None
    for tu in ("lazy_exact", "sparse_rows"):
        losses, st, n_steps = results[tu]
        if n_steps == 3:
            want_l, want_s = dense_l, dense_s
        else:
            if dense1 is None:
                m, c, _, _ = full_model(E, tu="dense_exact")
                m.load_state_dict(state)
                dense1 = run_steps(m, kind, c, batches[:1], graph)
            want_l, want_s = dense1
        assert np.allclose(losses, want_l, rtol=RTOL), (tu, losses, want_l)
        for k in st:
            b0 = before[k] if before[k].ndim else before[k].reshape(1)
            if k.startswith("embedding_dict."):
                moved = np.nonzero((want_s[k] != before[k]).any(1))[0]
                if kind == "adagrad" or tu == "lazy_exact":
                    idle = np.ones(b0.shape[0], bool)
                    idle[moved] = False
                    assert np.array_equal(st[k][idle], want_s[k][idle]), (tu, k)  # rows no batch touched
                rows = moved
                if rows.size == 0:
                    continue
            else:
                rows = np.arange(b0.shape[0])
            share, r = table_update_report(b0, st[k].reshape(b0.shape), want_s[k].reshape(b0.shape), rows)
            assert share < 2e-3, (tu, k, share, r)


def test_fit_learns_from_the_history_column_and_predict_round_trips():
    from mmlrec_amd.model.utils import get_feature_names
    E = 8
    model, cfg, cols, fi = full_model(E)
    rng = np.random.default_rng(21)
    N = 2048
    X = make_x(cols, fi, N, rng)
    a, b = fi["cats"]
    signal = (X[:, a:b] == 3).any(1)  # the label depends on the multi-valued column
    y = np.stack([signal, signal ^ (rng.random(N) < 0.1)], 1).astype(np.float32)
    x = {}
    for name in get_feature_names(cols):
        lo, hi = fi[name]
        x[name] = X[:, lo] if hi - lo == 1 else X[:, lo:hi]  # a sequence column is a 2-D [N, maxlen] entry
    model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
    model.fit(x, y, batch_size=256, epochs=3)
    losses = [e["loss"] for e in model.history]
    assert all(np.isfinite(losses)) and losses[1] < losses[0], losses
    p1 = model.predict(x, batch_size=256)
    twin, _, _, _ = full_model(E)
    twin.load_state_dict(model.state_dict())
    assert np.array_equal(twin.predict(x, batch_size=256), p1)


def test_refusals():
    from mmlrec_amd import parallel
    from mmlrec_amd.model import DenseFeat, SparseFeat, VarLenSparseFeat
    E = 8
    model, cfg, cols, fi = full_model(E)
    with pytest.raises(NotImplementedError):
        parallel.shard_model(model, None, 64)
    model, cfg, cols, fi = full_model(E)
    model.scatter_mode = "deterministic"
    model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
    model.train()
    with pytest.raises(NotImplementedError):
        model.train_step_runner(64, use_graph=False)
    # split dense update on request: the other schedule is picked, nothing fails
    model, cfg, cols, fi = full_model(E)
    model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
    model.train()
    step = model.train_step_runner(64, use_graph=False, split_dense="force")
    assert getattr(step.plan.ops[0], "mark_rows", None) is None
    # PepNet: a pooled feature declared before the scene feature
    pcfg = config("pepnet_amazon", emb=E)
    hist = VarLenSparseFeat(SparseFeat("hist", 30, embedding_dim=E), maxlen=4)
    scene, other = SparseFeat("scene", 2, embedding_dim=E), SparseFeat("s1", 12, embedding_dim=E)
    with pytest.raises(NotImplementedError):
        make_model("PepNet", [hist, scene, other], pcfg)
    make_model("PepNet", [scene, other, hist], pcfg)  # pooled features after the single-valued ones: accepted
    with pytest.raises(ValueError):  # a shared table with two sizes
        make_model("MMOE", [SparseFeat("item", 40, embedding_dim=E),
                            VarLenSparseFeat(SparseFeat("h", 41, embedding_dim=E, embedding_name="item"), 4),
                            DenseFeat("d", 1)], config(emb=E))


def test_default_path_records_todays_gather_and_scatter():
    from test_models_gpu import build, load_state
    from mmlrec_amd import engine
    g = load_golden("mmoe_ae30")
    model, cfg = build(g, table_update="dense_exact")
    load_state(model, g)
    model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
    model.train()
    step = model.train_step_runner(64, use_graph=False)
    gop = step.plan.ops[0]
    assert type(gop) is engine.GatherOp
    names = set()

    def collect(obj, depth=0):  # every recorded call list of the plan and of the step's launch segments
        if isinstance(obj, (list, tuple)):
            if len(obj) >= 2 and isinstance(obj, tuple) and hasattr(obj[0], "__name__") and isinstance(obj[1], tuple):
                names.add(obj[0].__name__)
            elif depth < 4:
                for o in obj:
                    collect(o, depth + 1)
        elif depth < 3 and hasattr(obj, "__dict__") and type(obj).__module__.startswith("mmlrec"):
            for v in vars(obj).values():
                collect(v, depth + 1)

    collect(step)
    collect(step.plan)
    # Recorded calls of the train step (one C call = one launch), counted over the step's launch segments.  The figures
    # were MEASURED on the parent commit's package (this fixture, Adam, B = 64, graph off and on alike): dense_exact 40,
    # lazy_exact 44, sparse_rows 40.
    from mmlrec_amd import trainer
    for tu, want in (("dense_exact", 40), ("lazy_exact", 44), ("sparse_rows", 40)):
        m, c = build(g, table_update=tu)
        load_state(m, g)
        m.compile("adam", c["optim_config"]["loss"], ["auc"])
        m.train()
        st = m.train_step_runner(64, use_graph=False)
        n = sum(sum(len(p[1]) if p[0] == "c" else 1 for p in v.parts)
                for v in vars(st).values() if isinstance(v, trainer.Segments))
        assert n == want, (tu, n, want)
    assert any(n.startswith("mml_gather_fwd") for n in names) and "mml_scatter_bwd" in names
    assert not any("pool" in n for n in names)


# ---------------------------------------------------------------------------------------------------------------
# Against fixtures made from the unmodified reference (tests/golden/make_golden_pooled.py -> tests/golden/pooled_*.npz)
# ---------------------------------------------------------------------------------------------------------------
POOLED_CASES = ["pooled_mmoe_mtl", "pooled_pepnet_mtmsl", "pooled_mmoe_e16", "pooled_sharedbottom_sum"]


def build_pooled(g, **model_kw):
    from mmlrec_amd.model import DenseFeat, SparseFeat, VarLenSparseFeat
    cfg = json.loads(str(g["cfg"]))
    cfg["model_config"].update(model_kw)
    emb = cfg["model_config"]["emb"]
    cols = [SparseFeat(str(n), int(v), embedding_dim=emb) for n, v in zip(g["sparse_names"], g["vocab"])]
    for p in json.loads(str(g["columns"])):  # pooled features after all single-valued ones, dense columns last
        cols.append(VarLenSparseFeat(SparseFeat(p["name"], int(p["vocab"]), embedding_dim=emb,
                                                embedding_name=p["shared_with"] or p["name"]),
                                     maxlen=int(p["maxlen"]), combiner=p["combiner"], length_name=p["length_name"]))
    cols += [DenseFeat(str(n), 1) for n in g["dense_names"]]
    cls = {"mmoe": "MMOE", "pepnet": "PepNet", "sharedbottom": "SharedBottom"}[cfg["model_config"]["model_name"]]
    return make_model(cls, cols, cfg), cfg, cols


def load_pooled_state(model, g):
    model.load_state_dict({k[6:]: torch.from_numpy(np.array(g[k])) for k in g.files if k.startswith("state/")},
                          strict=True)
    return model


def valid_rows(g, cols, upto=3):
    """{table key: sorted rows some valid position (or single-valued field) of batches 0..upto-1 names}"""
    from mmlrec_amd.model import SparseFeat, VarLenSparseFeat
    from mmlrec_amd.model.utils import build_input_features
    fi = build_input_features(cols)
    rows = {}
    for i in range(upto):
        X = g[f"X{i}"]
        for f in cols:
            if isinstance(f, SparseFeat):
                r = X[:, fi[f.name][0]].astype(np.int64)
            elif isinstance(f, VarLenSparseFeat):
                ids = X[:, fi[f.name][0]:fi[f.name][1]].astype(np.int64)
                if f.length_name is None:
                    ok = ids != 0
                else:
                    ok = np.arange(f.maxlen)[None, :] < X[:, fi[f.length_name][0]].astype(np.int64)[:, None]
                r = ids[ok]
            else:
                continue
            rows.setdefault(f"embedding_dict.{f.embedding_name}.weight", set()).update(r.tolist())
    return {k: np.array(sorted(v), np.int64) for k, v in rows.items()}


@pytest.fixture(params=POOLED_CASES)
def pcase(request):
    return request.param, load_golden(request.param)


@pytest.fixture(params=["fp16x2", "bf16x3"])
def arith(request, monkeypatch):
    """GEMM arithmetic of the recorded plans, as in tests/test_models_gpu.py."""
    monkeypatch.setenv("MMLREC_AMAX", "1" if request.param == "fp16x2" else "0")
    return request.param


def test_fixture_state_dict_and_seeded_init(pcase):
    name, g = pcase
    model, _, _ = build_pooled(g)
    want = {k[6:]: g[k].shape for k in g.files if k.startswith("state/")}
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert set(got) == set(want)  # a shared table has ONE key
    for k in want:
        assert got[k] == tuple(want[k]), k
    model.train()
    with torch.no_grad():
        y = model(torch.from_numpy(g["X0"]).cuda())
    assert rel(y.cpu().numpy(), g["init_y_pred"]) < RTOL


def test_fixture_forward_layers_mask_dnn_input(pcase):
    from mmlrec_amd.model.utils import build_input_features
    name, g = pcase
    model, cfg, cols = build_pooled(g)
    load_pooled_state(model, g)
    model.eval()
    model.update_save(True)
    X = torch.from_numpy(g["X0"]).cuda()
    with torch.no_grad():
        y = model(X)
    print(f"[{name}] y_pred rel={rel(y.cpu().numpy(), g['y_pred']):.3g} elem_rel={elem_rel(y.cpu().numpy(), g['y_pred']):.3g}")
    assert rel(y.cpu().numpy(), g["y_pred"]) < RTOL
    assert elem_rel(y.cpu().numpy(), g["y_pred"]) <= 1.0
    lo = model.layer_output_dict
    for k in g.files:
        if k.startswith("layer/"):
            assert rel(lo[k[6:]].cpu().numpy(), g[k]) < RTOL, k
    if "y_pred_masked" in g.files:
        with torch.no_grad():
            ym = model(X, torch.from_numpy(g["mask0"]).cuda())
        assert rel(ym.cpu().numpy(), g["y_pred_masked"]) < RTOL
    # dnn_input against the reference's float64 one: copies and max blocks bit-exact, sum / mean blocks inside the
    # worst-case bound of an fp32 summation (the bound needs sum |row|: taken from this file's float64 restatement,
    # which is itself held to the reference's float64 dnn_input first)
    fi = build_input_features(cols)
    t64 = {k.split(".")[1]: torch.from_numpy(g["state/" + k]).double() for k in model.state_dict()
           if k.startswith("embedding_dict.")}
    mine, bound = reference64(cols, fi, t64, g["X0"])
    ref64 = g["dnn_input64"]
    assert np.abs(mine.numpy() - ref64).max() <= 1e-12 * max(1.0, np.abs(ref64).max())
    got = lo["dnn_input"].cpu().numpy()
    exact = (bound == 0).numpy()
    assert np.array_equal(got[exact], ref64.astype(np.float32)[exact])
    assert np.all(np.abs(got.astype(np.float64) - ref64) <= bound.numpy())


def test_fixture_autograd_gradients(pcase, arith):
    name, g = pcase
    model, cfg, cols = build_pooled(g)
    load_pooled_state(model, g)
    model.train()
    X, y = torch.from_numpy(g["X0"]).cuda(), torch.from_numpy(g["y0"]).cuda()
    yp = model(X)
    bce = torch.nn.functional.binary_cross_entropy
    loss = sum(bce(yp[:, i], y[:, i], reduction="sum") for i in range(yp.shape[1]))
    (loss + model.get_regularization_loss().sum()).backward()
    assert abs(float(loss) - float(g["loss"])) / float(g["loss"]) < RTOL
    for n, p in model.named_parameters():
        if "grad64/" + n in g.files:
            assert p.grad is not None, n
            r = rel(p.grad.cpu().numpy(), g["grad64/" + n])
            assert r < RTOL, (n, r)
            if n.startswith("embedding_dict."):
                er = elem_rel(p.grad.cpu().numpy(), g["grad64/" + n])
                print(f"[{name} {arith}] {n}: rel={r:.3g} elem_rel={er:.3g}")
                assert er <= 1.0, (n, er)
        else:
            assert "nograd/" + n in g.files, n


@pytest.mark.parametrize("graph", [False, True])
def test_fixture_fused_train_steps(pcase, graph):
    """Step 1 of every (optimizer, table_update) pair the fixture pins against the reference's parameters after its
    first step (update criterion of conftest.table_update_report at share < 2e-3; rows no batch names must not move);
    the three losses; later pinned steps inside the absolute bound of tests/test_models_gpu.py's trajectory test
    (2.5 lr per step; 25 lr for RMSprop, whose step is up to 10 lr per element)."""
    name, g = pcase
    combos = [("adam", "dense_exact"), ("adam", "lazy_exact"), ("adagrad", "sparse_rows"), ("rmsprop", "dense_exact"),
              ("sgd", "sparse_rows")]
    combos = [c for c in combos if f"{c[0]}_losses" in g.files]
    assert combos
    for kind, tu in combos:
        model, cfg, cols = build_pooled(g, table_update=tu)
        load_pooled_state(model, g)
        model.optim_config["optimizer"] = kind
        model.compile(kind, cfg["optim_config"]["loss"], ["auc", "acc"])
        model.train()
        assert model.optimizer().table_update == tu
        lr = cfg["optim_config"]["lr"]
        before = {k[6:]: g[k] for k in g.files if k.startswith("state/")}
        losses = []
        for i in range(3):
            step = model.train_step_runner(64, use_graph=graph)
            step.plan.X.copy_(torch.from_numpy(g[f"X{i}"]).cuda())
            step.plan.y.copy_(torch.from_numpy(g[f"y{i}"]).cuda())
            step.run()
            losses.append(float(step.plan.loss.item()))
            if f"{kind}{i + 1}/{next(iter(before))}" not in g.files:
                continue
            sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
            touched = valid_rows(g, cols, upto=i + 1)
            for k, got in sd.items():
                ref = g[f"{kind}{i + 1}/{k}"]
                assert np.abs(got.astype(np.float64) - ref).max() <= (25.0 if kind == "rmsprop" else 2.5) * lr * (i + 1), \
                    (kind, tu, i + 1, k)
                if k in touched:
                    idle = np.ones(got.shape[0], bool)
                    idle[touched[k]] = False
                    assert np.array_equal(got[idle], before[k][idle]), (kind, tu, k, "a row no batch names moved")
                if i > 0:
                    continue
                b0 = before[k] if before[k].ndim else before[k].reshape(1)
                rows = touched[k] if k in touched else np.arange(b0.shape[0])
                share, r = table_update_report(b0, got.reshape(b0.shape), ref.reshape(b0.shape), rows)
                assert share < 2e-3, (kind, tu, k, share, r)
        assert np.allclose(losses, g[f"{kind}_losses"], rtol=RTOL), (kind, tu, losses, g[f"{kind}_losses"])


def test_evaluate_on_a_pooled_schema():
    from mmlrec_amd.model.utils import get_feature_names
    g = load_golden("pooled_mmoe_mtl")
    model, cfg, cols = build_pooled(g)
    load_pooled_state(model, g)
    from mmlrec_amd.model.utils import build_input_features
    fi = build_input_features(cols)
    X = np.concatenate([g["X0"], g["X1"], g["X2"]])
    y = np.concatenate([g["y0"], g["y1"], g["y2"]])
    x = {n: (X[:, fi[n][0]] if fi[n][1] - fi[n][0] == 1 else X[:, fi[n][0]:fi[n][1]]) for n in get_feature_names(cols)}
    model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
    res = model.evaluate(x, y, batch_size=64)
    assert res and all(np.isfinite(v) for v in res.values()), res
    p = model.predict(x, batch_size=64)
    assert rel(p[:64], g["y_pred"]) < RTOL


def test_main_trains_and_evaluates_a_config_with_sequence_columns(tmp_path):
    """End to end through the driver: JSON config with data_config["sequence_columns"] -> ctrdataset -> fit with
    validation -> predict -> result row (a history sharing the movie table by length column, tags of their own)."""
    import os
    import sys
    import pandas as pd
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import synth_csv
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import main as M
    tr, te = synth_csv.make_frames(n_train=2048, n_test=512)
    rng = np.random.default_rng(4)
    for df in (tr, te):
        movies = df["movie_tag"].to_numpy()
        hist, tags = [], []
        for i in range(len(df)):
            n = int(rng.integers(0, 12))  # longer than maxlen sometimes: the last 8 are kept
            hist.append("|".join(str(v) for v in rng.choice(movies, n)))
            # (at least one tag: an EMPTY sequence pooled by max is float32(row - 1e9) in the reference and here, an
            # input no network trains on)
            tags.append("|".join(f"t{v}" for v in rng.integers(0, 15, int(rng.integers(1, 5)))))
        df["hist"], df["tags"] = hist, tags
    a, b = str(tmp_path / "train.csv"), str(tmp_path / "test.csv")
    tr.to_csv(a, index=False)
    te.to_csv(b, index=False)
    res = tmp_path / "res.csv"
    cfg = synth_csv.config(a, b, str(res), "mmoe")
    cfg["data_config"]["all_columns"] = synth_csv.COLUMNS + ["hist", "tags"]
    cfg["data_config"]["sequence_columns"] = [
        {"name": "hist", "maxlen": 8, "combiner": "mean", "sep": "|", "shared_with": "movie_tag"},
        {"name": "tags", "maxlen": 4, "combiner": "max", "sep": "|"}]
    cfg["training_config"]["epochs"] = 1
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg))
    rows = M.run(M.build_parser().parse_args(["--config", str(p), "--run", "1", "--model_name", "mmoe", "--seeds", "0"]))
    assert len(rows) == 1 and 0.5 < rows[0]["auc_0"] <= 1.0 and 0.0 < rows[0]["log_loss_0"] < 1.0
    assert len(pd.read_csv(res)) == 1
