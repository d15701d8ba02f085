"""Regression tasks (task_types "regression", losses "mse" / "mae") through BaseModel, the engine, the fused train step
and the harness.

Against fixtures made from the unmodified reference (tests/golden/make_golden_regression.py -> tests/golden/reg_*.npz):
state keys and seeded init, predictions (masked too), loss and every gradient through autograd in both GEMM arithmetics
(1e-4 max-norm as in tests/test_models_gpu.py; table gradients by the element rule of tests/test_pooled_models_gpu.py),
and fused steps against the stored trajectories for the optimizer / table_update pairs the pooled tests use.

Full size: an AE-30-shaped MMoE with [binary, regression] at B = 32 768 with graphs on takes the fused tower + head launch;
three steps against the same model under MMLREC_TOWER_HEAD=0; the first step's loss and MLP gradients against a float64
torch restatement of the model on the device.  The gradients are read off ONE SGD step with lr = 0.1, g = (p0 - p1) / lr:
the update rounds once in fp32, so g carries at most ulp(max(|p0|, |p1|)) / (2 lr) of noise -- 3e-7 absolute for |p| < 1, or
6e-8 of g where the update dominates the parameter.  Against the 1e-4 max-norm criterion that is below a tenth of the
allowance for every tensor whose largest gradient exceeds 0.03, which the test asserts (the gradients are sums over
32 768 samples).
"""
import copy
import json

import numpy as np
import pytest
import torch

from conftest import load_golden, randomize_he, table_update_report
from test_models_gpu import build, elem_rel, load_state, rel

pytestmark = pytest.mark.gpu

RTOL = 1e-4
REG_CASES = ["reg_mmoe_mtl", "reg_ple", "reg_pepnet_mtmsl", "reg_star_msl", "reg_sharedbottom", "reg_mmoe_seconds"]
TORCH_LOSS = {"binary_crossentropy": torch.nn.functional.binary_cross_entropy, "mse": torch.nn.functional.mse_loss,
              "mae": torch.nn.functional.l1_loss}


@pytest.fixture(params=REG_CASES)
def rcase(request):
    return request.param, load_golden(request.param)


@pytest.fixture(params=["fp16x2", "bf16x3"])
def arith(request, monkeypatch):
    """GEMM arithmetic of the recorded plans, as in tests/test_models_gpu.py."""
    monkeypatch.setenv("MMLREC_AMAX", "1" if request.param == "fp16x2" else "0")
    return request.param


def touched_rows(g, model, upto=3):
    from mmlrec_amd.model import SparseFeat
    rows = {}
    for i in range(upto):
        X = g[f"X{i}"]
        for f in model.dnn_feature_columns:
            if isinstance(f, SparseFeat):
                r = X[:, model.feature_index[f.name][0]].astype(np.int64)
                rows.setdefault(f"embedding_dict.{f.embedding_name}.weight", set()).update(r.tolist())
    return {k: np.array(sorted(v), np.int64) for k, v in rows.items()}


def test_fixture_state_dict_and_seeded_init(rcase):
    name, g = rcase
    model, cfg = build(g)
    want = {k[6:]: g[k].shape for k in g.files if k.startswith("state/")}
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert set(got) == set(want)
    for k in want:
        assert got[k] == tuple(want[k]), k
    model.train()
    with torch.no_grad():
        y = model(torch.from_numpy(g["X0"]).cuda())
    print(f"[{name}] init_y_pred rel={rel(y.cpu().numpy(), g['init_y_pred']):.3g}")
    assert rel(y.cpu().numpy(), g["init_y_pred"]) < RTOL


def test_fixture_forward_and_mask(rcase, arith):
    name, g = rcase
    model, cfg = build(g)
    load_state(model, g)
    model.eval()
    X = torch.from_numpy(g["X0"]).cuda()
    with torch.no_grad():
        y = model(X).cpu().numpy()
    print(f"[{name} {arith}] y_pred rel={rel(y, g['y_pred64']):.3g}")
    assert rel(y, g["y_pred"]) < RTOL and rel(y, g["y_pred64"]) < RTOL
    for t in range(y.shape[1]):  # column by column: a regression column is not hidden behind a larger one
        assert rel(y[:, t], g["y_pred64"][:, t]) < RTOL, t
    if "y_pred_masked" in g.files:
        with torch.no_grad():
            ym = model(X, torch.from_numpy(g["mask0"]).cuda()).cpu().numpy()
        assert rel(ym, g["y_pred_masked"]) < RTOL
    # predict() returns the raw values of the regression columns
    p = model.predict(g["X0"], batch_size=64)
    assert p.dtype == np.float64 and rel(p, g["y_pred"]) < RTOL


def test_fixture_autograd_gradients(rcase, arith):
    name, g = rcase
    model, cfg = build(g)
    load_state(model, g)
    model.train()
    X, y = torch.from_numpy(g["X0"]).cuda(), torch.from_numpy(g["y0"]).cuda()
    yp = model(X)
    names = cfg["optim_config"]["loss"]
    loss = sum(TORCH_LOSS[names[i]](yp[:, i], y[:, i], reduction="sum") for i in range(yp.shape[1]))
    (loss + model.get_regularization_loss().sum()).backward()
    print(f"[{name} {arith}] loss rel={abs(float(loss) - float(g['loss64'])) / float(g['loss64']):.3g}")
    assert abs(float(loss) - float(g["loss"])) / float(g["loss"]) < RTOL
    assert abs(float(loss) - float(g["loss64"])) / float(g["loss64"]) < RTOL
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
def test_fixture_fused_train_steps(rcase, arith, graph):
    """The labelled path of the head kernels (loss kinds included) through the fused step: step 1 against the
    reference's parameters after its first step (update criterion of conftest.table_update_report at share < 2e-3; rows no
    batch names must not move), the three losses, step 3 inside 2.5 lr per step."""
    name, g = rcase
    combos = [c for c in (("adam", "dense_exact"), ("adam", "lazy_exact"), ("adagrad", "sparse_rows"))
              if f"{c[0]}_losses" in g.files]
    assert combos
    for kind, tu in combos:
        model, cfg = build(g, table_update=tu)
        load_state(model, g)
        model.optim_config["optimizer"] = kind
        model.compile(kind, cfg["optim_config"]["loss"], ["mse"])
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
            touched = touched_rows(g, model, upto=i + 1)
            for k, got in sd.items():
                ref = g[f"{kind}{i + 1}/{k}"]
                assert np.abs(got.astype(np.float64) - ref).max() <= 2.5 * lr * (i + 1), (kind, tu, i + 1, k)
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
        print(f"[{name} {arith} {kind}/{tu} graph={graph}] losses {losses} ref {list(g[f'{kind}_losses'])}")
        assert np.allclose(losses, g[f"{kind}_losses"], rtol=RTOL), (kind, tu, losses, g[f"{kind}_losses"])


# ---------------------------------------------------------------------------------------------------------------
# full size
# ---------------------------------------------------------------------------------------------------------------
def ae30_regression(lr=None, optimizer="adam"):
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import workloads
    model, cfg, vocab, dense = workloads.build_model(
        "mmoe_ae30", torch.device("cuda:0"), vocab_scale=0.01, task_name="mtl", task_names=["ctr", "watch"],
        task_types=["binary", "regression"], table_update="dense_exact")
    cfg["optim_config"].update(loss=["binary_crossentropy", "mse"], optimizer=optimizer)
    if lr is not None:
        cfg["optim_config"]["lr"] = lr
    randomize_he(model, 7)
    return model, cfg, vocab


def ae30_batches(vocab, B, n):
    from mmlrec_amd import workloads
    out = []
    for i in range(n):
        X, y = workloads.synth_batch(vocab, 0, B, 2, seed=100 + i)
        g = torch.Generator().manual_seed(200 + i)
        y[:, 1] = 0.1 + 2.0 * torch.rand(B, generator=g)  # a watch ratio beside the click label
        out.append((X.cuda(), y.cuda()))
    return out


def mmoe64(sd, names, X, y):
    """float64 restatement of the MMoE (reference model/mmoe.py:65-108) with PredictionLayer("binary") on task 0 and
    PredictionLayer("regression") on task 1, BCE + MSE summed over the batch; returns (loss, {name: gradient})."""
    P = {k: v.detach().double().clone().requires_grad_(not k.startswith("embedding_dict.")) for k, v in sd.items()}
    x0 = torch.cat([P[f"embedding_dict.{n}.weight"][X[:, i].long()] for i, n in enumerate(names)], 1)

    def dnn(prefix, x):
        layer = 0
        while f"{prefix}.linears.{layer}.weight" in P:
            x = torch.relu(x @ P[f"{prefix}.linears.{layer}.weight"].t() + P[f"{prefix}.linears.{layer}.bias"])
            layer += 1
        return x

    ne = len([k for k in P if k.startswith("expert_dnn.") and k.endswith("linears.0.weight")])
    experts = torch.stack([dnn(f"expert_dnn.{e}", x0) for e in range(ne)], 1)
    preds = []
    for t in range(2):
        gate = torch.softmax(dnn(f"gate_dnn.{t}", x0) @ P[f"gate_dnn_final_layer.{t}.weight"].t(), -1)
        mix = (gate[:, :, None] * experts).sum(1)
        z = dnn(f"tower_dnn.{t}", mix) @ P[f"tower_dnn_final_layer.{t}.weight"].t() + P[f"out.{t}.bias"]
        preds.append(z[:, 0])
    p0 = torch.sigmoid(preds[0])
    y = y.double()
    loss = torch.nn.functional.binary_cross_entropy(p0, y[:, 0], reduction="sum") + ((preds[1] - y[:, 1]) ** 2).sum()
    loss.backward()
    return float(loss), {k: v.grad for k, v in P.items() if v.requires_grad}, torch.stack([p0, preds[1]], 1).detach()


def test_full_size_mmoe_takes_the_fused_launch_and_matches_float64(monkeypatch):
    B = 32768
    # (a) Adam, graphs on: fused against MMLREC_TOWER_HEAD=0 over three steps
    runs = {}
    for fused in (True, False):
        monkeypatch.setenv("MMLREC_TOWER_HEAD", "1" if fused else "0")
        model, cfg, vocab = ae30_regression()
        state0 = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
        model.compile("adam", cfg["optim_config"]["loss"], ["auc", "mse"])
        model.train()
        step = model.train_step_runner(B, use_graph=True)
        assert (step.plan.tower_head is not None) == fused
        if fused:
            assert int(step.plan.tower_head.t[0].kind) == 0 and int(step.plan.tower_head.t[1].kind) == 0x101
        losses = []
        for X, y in ae30_batches(vocab, B, 3):
            step.plan.X.copy_(X)
            step.plan.y.copy_(y)
            step.run()
            losses.append(float(step.plan.loss.item()))
            if len(losses) == 1:
                first = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
        runs[fused] = (losses, first, {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()})
        del step, model
    monkeypatch.delenv("MMLREC_TOWER_HEAD")
    (lf, f1, f3), (lu, u1, u3) = runs[True], runs[False]
    print("losses fused", lf, "three launches", lu)
    assert np.allclose(lf, lu, rtol=RTOL)
    lr = cfg["optim_config"]["lr"]
    for k in f1:
        if k.startswith("embedding_dict."):
            rows = np.nonzero((u1[k] != state0[k]).any(1))[0]
            if rows.size == 0:
                continue
        else:
            rows = np.arange(state0[k].shape[0]) if state0[k].ndim else np.arange(1)
        b0 = state0[k] if state0[k].ndim else state0[k].reshape(1)
        share, r = table_update_report(b0, f1[k].reshape(b0.shape), u1[k].reshape(b0.shape), rows)
        assert share < 2e-3, (k, share, r)
        assert np.abs(f3[k].astype(np.float64) - u3[k]).max() <= 2.5 * lr * 3, k
    # (b) the first step's loss and MLP gradients against float64: one SGD step, g = (p0 - p1) / lr
    lr = 0.1
    model, cfg, vocab = ae30_regression(lr=lr, optimizer="sgd")
    model.optim_config.update(lr=lr, optimizer="sgd")
    names = [f.embedding_name for f in model.dnn_feature_columns]
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.compile("sgd", cfg["optim_config"]["loss"], ["mse"])
    model.train()
    step = model.train_step_runner(B, use_graph=True)
    assert step.plan.tower_head is not None
    X, y = ae30_batches(vocab, B, 1)[0]
    step.plan.X.copy_(X)
    step.plan.y.copy_(y)
    step.run()
    loss = float(step.plan.loss.item())
    pred = step.plan.prob.clone()
    sd1 = model.state_dict()
    loss64, grads64, pred64 = mmoe64(sd0, names, X, y)
    print(f"loss {loss} float64 {loss64} rel {abs(loss - loss64) / loss64:.3g}")
    assert abs(loss - loss64) / loss64 < RTOL
    for t in range(2):
        assert rel(pred[:, t].cpu().numpy(), pred64[:, t].cpu().numpy()) < RTOL, t
    for k, g64 in grads64.items():
        got = (sd0[k].double() - sd1[k].double()) / lr
        r = float((got - g64).abs().max() / g64.abs().max().clamp_min(1e-30))
        print(f"  {k}: max|g|={float(g64.abs().max()):.3g} rel={r:.3g}")
        assert float(g64.abs().max()) > 0.03, k  # (the noise of reading g off the update stays below 1e-5 of it: docstring)
        assert r < RTOL, (k, r)


# ---------------------------------------------------------------------------------------------------------------
# harness
# ---------------------------------------------------------------------------------------------------------------
def small_model(task_types, losses, cls="MMOE", pooled=False, data_kw=None, **model_kw):
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import model as M
    from mmlrec_amd.model import DenseFeat, SparseFeat, VarLenSparseFeat
    cfg = json.loads(str(load_golden("mmoe_kuairec")["cfg"]))
    cfg["model_config"].update(emb=8, task_names=["ctr", "watch"], task_types=list(task_types), **model_kw)
    cfg["optim_config"].update(loss=list(losses), lr=0.01)
    cfg["data_config"].update(data_kw or {})
    cols = [SparseFeat("user", 50, embedding_dim=8), SparseFeat("item", 200, embedding_dim=8)]
    if pooled:
        cols.append(VarLenSparseFeat(SparseFeat("hist", 200, embedding_dim=8, embedding_name="item"), maxlen=5,
                                     combiner="mean"))
    cols.append(DenseFeat("price", 1))
    torch.manual_seed(0)
    return getattr(M, cls)(cols, device="cuda:0", config=cfg), cfg, cols


def linear_data(N, seed, pooled=False):
    rng = np.random.default_rng(seed)
    x = {"user": rng.integers(0, 50, N).astype(np.float32), "item": rng.integers(1, 200, N).astype(np.float32)}
    if pooled:
        hist = rng.integers(1, 200, (N, 5)).astype(np.float32)
        hist[np.arange(5)[None, :] >= rng.integers(1, 6, N)[:, None]] = 0.0
        x["hist"] = hist
    price = rng.random(N).astype(np.float32)
    x["price"] = price
    watch = 3.0 * price + 0.5 + 0.05 * rng.standard_normal(N)  # depends linearly on the dense column
    click = (price + 0.2 * rng.standard_normal(N) > 0.5)
    return x, np.stack([click, watch], 1).astype(np.float32)


def test_fit_learns_a_linear_label_and_logs_auc_and_mse():
    model, cfg, cols = small_model(["binary", "regression"], ["binary_crossentropy", "mse"])
    x, y = linear_data(4096, 3)
    xv, yv = linear_data(1024, 4)
    model.compile("adam", cfg["optim_config"]["loss"], ["auc", "mse"])
    model.fit(x, y, batch_size=256, epochs=5, validation_data=(xv, yv))
    hist = model.history
    assert all("auc" in e and "mse" in e and "val_auc" in e and "val_mse" in e for e in hist)
    mses = [e["mse"] for e in hist]
    print("mse per epoch", mses, "val", [e["val_mse"] for e in hist], "auc", [e["auc"] for e in hist])
    assert all(np.isfinite(mses)) and mses[-1] < 0.25 * mses[0], mses
    assert hist[-1]["val_mse"] < 0.25 * hist[0]["mse"] and hist[-1]["auc"] > 0.7
    # evaluate() (the host path) agrees with plain numpy on the metric's own columns; the device metrics of the epoch log are
    # held to per-batch sklearn values in test_device_batch_metrics_are_the_per_batch_sklearn_values
    p = model.predict(xv, batch_size=256)
    res = model.evaluate(xv, yv, batch_size=256)
    assert abs(res["mse"] - float(((p[:, 1] - yv[:, 1]) ** 2).mean())) < 1e-9
    from sklearn.metrics import roc_auc_score
    assert abs(res["auc"] - roc_auc_score(yv[:, 0], p[:, 0])) < 1e-12
    assert p[:, 1].max() > 1.5  # raw values, not probabilities
    # round trips
    twin, _, _ = small_model(["binary", "regression"], ["binary_crossentropy", "mse"])
    twin.load_state_dict(model.state_dict())
    assert np.array_equal(twin.predict(xv, batch_size=256), p)
    assert np.array_equal(copy.deepcopy(model).predict(xv, batch_size=256), p)


@pytest.mark.parametrize("mode", ["mtl", "mtmsl", "msl"])
def test_device_batch_metrics_are_the_per_batch_sklearn_values(mode):
    """_device_batch_metrics (auc / acc / mse of every batch of an epoch, on the device, averaged over the steps) against
    sklearn applied batch by batch to the same permutation through _metric, the host path -- with the two kinds of column
    on deliberately different scales, so that a metric reading the wrong column cannot agree."""
    from sklearn.metrics import mean_squared_error, roc_auc_score
    rng = np.random.default_rng(5)
    N, bs = 1000, 128  # (a ragged last batch)
    click = (rng.random(N) < 0.4).astype(np.float32)
    watch = (50.0 + 100.0 * rng.random(N)).astype(np.float32)
    pc = np.clip(0.3 * click + 0.7 * rng.random(N), 0, 1).astype(np.float32)
    pw = (watch + 10.0 * rng.standard_normal(N)).astype(np.float32)
    if mode == "mtl":
        model, cfg, _ = small_model(["binary", "regression"], ["binary_crossentropy", "mse"])
        y, p = np.stack([click, watch], 1), np.stack([pc, pw], 1)
        metrics = ["auc", "acc", "mse"]
    elif mode == "mtmsl":  # two label groups of two domains: the heads of a group sum to the group's prediction
        model, cfg, _ = small_model(["binary", "binary", "regression", "regression"], ["binary_crossentropy"] * 2 + ["mse"] * 2,
                                    task_name="mtmsl", data_kw=dict(label_columns=["l", "l", "w", "w"], num_domains=2,
                                                                    mask_values=[0, 1], mask_column="user",
                                                                    scene_feature="user"))
        y, p = np.stack([click, click, watch, watch], 1), np.stack([0.3 * pc, 0.7 * pc, 0.4 * pw, 0.6 * pw], 1)
        metrics = ["auc", "acc", "mse"]
    else:  # msl, all regression: one summed column
        model, cfg, _ = small_model(["regression", "regression"], ["mse", "mse"], task_name="msl",
                                    data_kw=dict(label_columns=["w", "w"], num_domains=2, mask_values=[0, 1],
                                                 mask_column="user", scene_feature="user"))
        y, p = np.stack([watch, watch], 1), np.stack([0.4 * pw, 0.6 * pw], 1)
        metrics = ["mse"]
    model.compile("adam", cfg["optim_config"]["loss"], metrics)
    perm = rng.permutation(N)
    yd, perm_d = torch.from_numpy(y).cuda(), torch.from_numpy(perm).cuda()
    pred = torch.from_numpy(p[perm]).cuda()  # (fit stores the predictions in the epoch's order)
    got = model._device_batch_metrics(pred, yd, perm_d, bs)
    assert set(got) == set(metrics)
    steps = (N - 1) // bs + 1
    ye, pe = y[perm].astype(np.float64), p[perm].astype(np.float64)
    for name in metrics:
        vals = [model._metric(model.metrics[name], ye[s * bs:(s + 1) * bs], pe[s * bs:(s + 1) * bs], model.metric_cols[name])
                for s in range(steps)]
        want = float(np.sum(vals)) / steps
        print(mode, name, got[name], want)
        assert abs(got[name] - want) <= 1e-6 * max(abs(want), 1.0), (mode, name, got[name], want)  # (fp32 inputs, fp64 sums)
    # ... and against sklearn written out for the mtl case, independently of _metric
    if mode == "mtl":
        auc = np.mean([roc_auc_score(ye[s * bs:(s + 1) * bs, 0], pe[s * bs:(s + 1) * bs, 0]) for s in range(steps)])
        mse = np.mean([mean_squared_error(ye[s * bs:(s + 1) * bs, 1], pe[s * bs:(s + 1) * bs, 1]) for s in range(steps)])
        assert abs(got["auc"] - auc) <= 1e-6 and abs(got["mse"] - mse) <= 1e-6 * mse
        assert mse > 50.0  # (the wrong column would give a value near 0.1 or near 1e4)


def test_fit_of_an_all_regression_model_selects_and_stops_on_val_mse():
    model, cfg, cols = small_model(["regression", "regression"], ["mse", "mae"])
    x, y = linear_data(4096, 3)
    xv, yv = linear_data(1024, 4)
    y2, yv2 = np.stack([y[:, 1], 2.0 * y[:, 1]], 1), np.stack([yv[:, 1], 2.0 * yv[:, 1]], 1)
    model.optim_config["early_stop"] = 2
    model.compile("adam", cfg["optim_config"]["loss"], ["mse"])
    best = model.fit(x, y2, batch_size=256, epochs=6, validation_data=(xv, yv2))
    vals = [e["val_mse"] for e in model.history]
    print("val_mse", vals)
    # a learning model is not cut off after `early_stop` epochs for want of an auc
    if len(vals) < 6:  # stopped early: only because the last two epochs did not improve on the best before them
        assert vals[-1] >= min(vals[:-2]) and vals[-2] >= min(vals[:-2]), vals
    assert vals[-1] < 0.5 * vals[0] and len(model.history) > 2
    # the returned model is the epoch with the lowest validation mse
    got = best.evaluate(xv, yv2, batch_size=256)["mse"]
    assert abs(got - min(vals)) <= 1e-9 * max(min(vals), 1.0), (got, vals)
    # without any metric to select on: no early stopping, the trained model itself comes back
    model, cfg, cols = small_model(["regression", "regression"], ["mse", "mae"])
    model.optim_config["early_stop"] = 1
    model.compile("adam", cfg["optim_config"]["loss"], [])
    assert model.fit(x, y2, batch_size=256, epochs=3, validation_data=(xv, yv2)) is model
    assert len(model.history) == 3


def test_pooled_column_with_a_regression_task():
    model, cfg, cols = small_model(["binary", "regression"], ["binary_crossentropy", "mae"], pooled=True)
    x, y = linear_data(2048, 5, pooled=True)
    model.compile("adam", cfg["optim_config"]["loss"], ["auc", "mse"])
    model.fit(x, y, batch_size=256, epochs=4)
    mses = [e["mse"] for e in model.history]
    assert all(np.isfinite(mses)) and mses[-1] < mses[0], mses
    # the same batch through autograd: the loss the fused step reports is torch's
    X = torch.from_numpy(model._as_matrix(x)[:256]).cuda()
    yd = torch.from_numpy(y[:256]).cuda()
    model.train()
    yp = model(X)
    want = float(torch.nn.functional.binary_cross_entropy(yp[:, 0], yd[:, 0], reduction="sum") +
                 torch.nn.functional.l1_loss(yp[:, 1], yd[:, 1], reduction="sum"))
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    step = model.train_step_runner(256, use_graph=False)
    step.plan.X.copy_(X)
    step.plan.y.copy_(yd)
    step.run()
    assert abs(float(step.plan.loss.item()) - want) / want < RTOL
    assert any(not torch.equal(v, before[k]) for k, v in model.state_dict().items())


def test_bf16_storage_mode_with_a_regression_task():
    """mml_gemm_set_mode(1) (bf16 operands and storage, outside the 1e-4 contract): the head kernel writes bf16 dH for
    heads of any kind.  Held against the fp32 model from the same state at the 2e-2 of an 8-bit significand over a few
    layers -- a smoke bound, stated as such: the kernel-level check of bf16 dH is in tests/test_regression_heads_gpu.py."""
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L
    lib = L.load()
    x, y = linear_data(512, 6)
    losses = {}
    mode0 = lib.mml_gemm_get_mode()
    try:
        for mode in (mode0, 1):
            lib.mml_gemm_set_mode(mode)
            model, cfg, cols = small_model(["binary", "regression"], ["binary_crossentropy", "mse"],
                                           expert_dnn_hidden_units=[64, 32], gate_dnn_hidden_units=[32],
                                           tower_dnn_hidden_units=[32])
            randomize_he(model, 3)
            model.compile("adam", cfg["optim_config"]["loss"], ["mse"])
            model.train()
            step = model.train_step_runner(512, use_graph=False)
            step.plan.X.copy_(torch.from_numpy(model._as_matrix(x)).cuda())
            step.plan.y.copy_(torch.from_numpy(y).cuda())
            ls = []
            for _ in range(3):
                step.run()
                ls.append(float(step.plan.loss.item()))
            losses[mode] = ls
            del step, model
    finally:
        lib.mml_gemm_set_mode(mode0)
    a, b = losses[mode0], losses[1]
    print("fp32-class", a, "bf16 storage", b)
    assert all(np.isfinite(b)) and b[2] < b[0]
    assert np.allclose(a, b, rtol=2e-2), (a, b)


def test_main_writes_mse_and_mae_for_a_regression_task(tmp_path):
    import os
    import sys
    import pandas as pd
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import synth_csv
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import main as M
    tr, te = synth_csv.make_frames(n_train=2048, n_test=512)
    rng = np.random.default_rng(4)
    for df in (tr, te):  # label3 becomes a continuous watch ratio that follows label2
        df["label3"] = 0.3 + 1.5 * df["label2"].to_numpy() + 0.1 * rng.standard_normal(len(df))
    a, b = str(tmp_path / "train.csv"), str(tmp_path / "test.csv")
    tr.to_csv(a, index=False)
    te.to_csv(b, index=False)
    res = tmp_path / "res.csv"
    cfg = synth_csv.config(a, b, str(res), "mmoe")
    cfg["model_config"].update(task_names=["ctr", "watch"], task_types=["binary", "regression"])
    cfg["optim_config"].update(loss=["binary_crossentropy", "mse"], metrics=["auc", "mse"])
    cfg["training_config"]["epochs"] = 2
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg))
    rows = M.run(M.build_parser().parse_args(["--config", str(p), "--run", "1", "--model_name", "mmoe", "--seeds", "0"]))
    assert len(rows) == 1
    row = rows[0]
    assert set(row) == {"type", "log_loss_0", "auc_0", "mse_1", "mae_1"}, row
    assert 0.5 < row["auc_0"] <= 1.0 and 0.0 <= row["mse_1"] < 1.0 and 0.0 <= row["mae_1"] < 1.0, row
    out = pd.read_csv(res)
    assert len(out) == 1 and "mse_1" in out.columns
    # ctrdataset handed the continuous label column through unchanged
    from mmlrec_amd.utils.data_utils import ctrdataset
    train = ctrdataset(cfg)[0]
    assert np.allclose(np.sort(train["label3"].to_numpy()), np.sort(tr["label3"].to_numpy()))


def test_refusals():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import model as M
    for cls in ("ESMM", "ESCM", "AITM"):
        with pytest.raises((NotImplementedError, ValueError)):
            small_model(["binary", "regression"], ["binary_crossentropy", "mse"], cls=cls)
        m, cfg, _ = small_model(["binary", "binary"], ["binary_crossentropy"] * 2, cls=cls)
        with pytest.raises(NotImplementedError):
            m.compile("adam", ["binary_crossentropy", "mse"], ["auc"])
        m.compile("adam", ["binary_crossentropy"] * 2, ["auc"])
    m, cfg, _ = small_model(["binary", "regression"], ["binary_crossentropy", "mse"])
    with pytest.raises(ValueError):  # identity output with BCE
        m.compile("adam", ["binary_crossentropy", "binary_crossentropy"], ["auc"])
    with pytest.raises(NotImplementedError):
        m.compile("adam", ["binary_crossentropy", "huber"], ["auc"])
    m.compile("adam", ["mse", "mae"], ["auc", "mse"])  # sigmoid + MSE is allowed
    m, cfg, _ = small_model(["regression", "regression"], ["mse", "mae"])
    with pytest.raises(ValueError):  # a metric without a column of its kind
        m.compile("adam", ["mse", "mae"], ["auc", "mse"])
    m.compile("adam", ["mse", "mae"], ["mse"])
    m, cfg, _ = small_model(["binary", "binary"], ["binary_crossentropy"] * 2)
    m.compile("adam", ["binary_crossentropy"] * 2, ["auc", "mse"])  # all binary: every metric scores every column, as before
    assert m.metric_cols == {"auc": None, "mse": None}
    assert M is not None
