"""The device_metrics switch through the models: evaluate(), fit() and the CLI's result row with
the switch on against the same calls with it off (the host path over sklearn)."""
import json
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, load_golden, randomize_he
from test_models_gpu import build, load_state

sys.path.insert(0, GOLDEN_DIR)
import synth_csv  # noqa: E402

pytestmark = pytest.mark.gpu

SKLEARN_TOL = 1e-12  # tests/test_kernels_gpu.py::test_auc_segments_match_sklearn


def synth_rows(g, n, seed):
    """n rows whose every column is drawn from the fixture's own values of that column (valid indices, valid domains)."""
    pool = np.concatenate([g["X0"], g["X1"], g["X2"]])
    rng = np.random.default_rng(seed)
    return np.stack([pool[rng.integers(0, len(pool), n), f] for f in range(pool.shape[1])], 1).astype(np.float32)


def synth_labels(model, n, seed):
    rng = np.random.default_rng(seed)
    cols = [(rng.random(n) < 0.35).astype(np.float32) if t == "binary" else rng.standard_normal(n).astype(np.float32)
            for t in model.task_types]
    if model.task_name in ("msl", "mtmsl"):  # one label per group, repeated for its domains
        D = model.num_domains
        cols = [cols[(i // D) * D] for i in range(len(cols))]
    return np.stack(cols, 1)


def same(a, b):
    return (a == b) or (a != a and b != b)


def count_auc_sorted(monkeypatch):
    """Calls of ops.auc_sorted from here on (a list that grows by one per call): the switch-on paths must reach the
    kernel, not fall back to the host."""
    from mmlrec_amd import ops
    calls, original = [], ops.auc_sorted

    def counted(*a, **k):
        calls.append(k.get("seg", a[2] if len(a) > 2 else 0))
        return original(*a, **k)

    monkeypatch.setattr(ops, "auc_sorted", counted)
    return calls


@pytest.mark.parametrize("name,metrics", [("mmoe_kuairec", ["auc", "acc", "logloss"]),
                                          ("star_dbn", ["auc", "acc", "logloss"]),
                                          ("pepnet_amazon", ["auc", "acc", "logloss"]),
                                          ("reg_mmoe_mtl", ["auc", "acc", "mse", "logloss"])])
def test_evaluate_on_the_device_equals_the_host_path(name, metrics, monkeypatch):
    g = load_golden(name)
    model, cfg = build(g)
    calls = count_auc_sorted(monkeypatch)
    load_state(model, g)
    randomize_he(model, 5)  # (the fixtures' 1e-4 init puts every probability next to 0.5)
    model.compile(cfg["optim_config"]["optimizer"], cfg["optim_config"]["loss"], metrics)
    assert model.device_metrics is False
    n = 3001
    X, y = synth_rows(g, n, 1), synth_labels(model, n, 2)
    torch.manual_seed(0)
    host = model.evaluate(X, y, batch_size=1024)
    pred = model.predict(X, batch_size=1024)
    assert calls == []
    model.device_metrics = True
    torch.manual_seed(0)
    got = model.evaluate(X, y, batch_size=1024)
    assert calls == [0]  # one call over the whole set
    assert np.array_equal(model.predict(X, batch_size=1024), pred) and pred.dtype == np.float64  # predict is unchanged
    assert list(got) == list(host)
    print(name, "host", host, "device", got)
    assert abs(got["auc"] - host["auc"]) < SKLEARN_TOL and 0.0 < host["auc"] < 1.0
    assert got["acc"] == host["acc"]
    assert same(got["logloss"], host["logloss"])  # the same host path: bit for bit
    if "mse" in metrics:
        pm = pred if model.metric_columns is None else pred[:, list(model.metric_columns)]
        c = model.metric_cols["mse"]
        terms = (y[:, c].astype(np.float64) - pm[:, c]) ** 2 / (n * len(c))
        bound = terms.size * 2.0 ** -52 * np.abs(terms).sum()  # a reordered float64 sum
        assert abs(got["mse"] - host["mse"]) <= bound, (got["mse"], host["mse"], bound)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("name", ["star_dbn", "pepnet_amazon", "mmoe_kuairec"])
def test_evaluate_with_a_non_finite_prediction_is_nan_on_both_paths(name, bad, monkeypatch):
    """A diverged model must not get a plausible val_auc: one NaN / infinite prediction makes `auc` NaN with the switch on
    as with it off (sklearn refuses the input, _metric reports NaN) -- also where the column is a float64 sum of heads
    (msl, mtmsl) that reaches the kernel as dense ranks."""
    g = load_golden(name)
    model, cfg = build(g)
    load_state(model, g)
    randomize_he(model, 5)
    model.compile(cfg["optim_config"]["optimizer"], cfg["optim_config"]["loss"], ["auc"])
    n = 2000
    X, y = synth_rows(g, n, 1), synth_labels(model, n, 2)
    calls = count_auc_sorted(monkeypatch)
    original = model._predict_device
    poison = [False]

    def predict_device(*a, **k):
        pred, layers = original(*a, **k)
        if poison[0]:
            pred = pred.clone()
            pred[7, 0] = bad
        return pred, layers

    monkeypatch.setattr(model, "_predict_device", predict_device)
    for switch in (False, True):
        model.device_metrics = switch
        poison[0] = False
        clean = model.evaluate(X, y, batch_size=1024)["auc"]
        assert 0.0 < clean < 1.0
        poison[0] = True
        assert np.isnan(model.evaluate(X, y, batch_size=1024)["auc"]), (name, bad, switch)
    assert calls == [0, 0]


def test_order_scores_keeps_order_ties_and_non_finite_values():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd.model.basemodel import BaseModel
    s = torch.tensor([0.3, float("nan"), 0.1, 0.3, float("inf"), 0.1 + 1e-12, -float("inf"), -2.0], dtype=torch.float64,
                     device="cuda")
    r = BaseModel._order_scores(s).cpu()
    assert r.dtype == torch.float32
    fin = torch.isfinite(s.cpu())
    assert torch.equal(torch.isfinite(r), fin)  # NaN and both infinities stay non-finite: the kernel flags them
    a, b = s.cpu()[fin], r[fin].view(torch.int32)
    for i in range(len(a)):
        for j in range(len(a)):
            assert (a[i] < a[j]) == (b[i] < b[j]) and (a[i] == a[j]) == (b[i] == b[j])


def test_evaluate_single_class_column_is_nan():
    g = load_golden("mmoe_kuairec")
    model, cfg = build(g)
    load_state(model, g)
    model.compile("adam", cfg["optim_config"]["loss"], ["auc"], device_metrics=True)
    X, y = synth_rows(g, 500, 1), synth_labels(model, 500, 2)
    y[:, 1] = 1.0
    assert np.isnan(model.evaluate(X, y, batch_size=256)["auc"])
    model.device_metrics = False
    assert np.isnan(model.evaluate(X, y, batch_size=256)["auc"])


def test_fit_with_large_batches(capsys, monkeypatch):
    """Two epochs at batch 5000 over 12 345 rows (a ragged last batch) with validation.  Deterministic scatter mode, so that
    the two runs train bit-identical models and the only difference is where the metrics are computed."""
    g = load_golden("mmoe_kuairec")
    n, nv, bs = 12345, 3000, 5000
    X, Xv = synth_rows(g, n, 3), synth_rows(g, nv, 4)
    runs = {}
    calls = count_auc_sorted(monkeypatch)
    for switch in (False, True):
        model, cfg = build(g, table_update="dense_exact")
        load_state(model, g)
        randomize_he(model, 6)
        model.scatter_mode = "deterministic"
        model.compile("adam", cfg["optim_config"]["loss"], ["auc", "acc"], device_metrics=switch)
        y, yv = synth_labels(model, n, 7), synth_labels(model, nv, 8)
        # labels the model can learn a little of, so that the epochs differ in val_auc
        y[:, 0] = (X[:, 0] % 2 == 0)
        yv[:, 0] = (Xv[:, 0] % 2 == 0)
        if not switch:  # today's behaviour: batches above 4096 rows go to the host
            probe = torch.rand(bs * 2, 2, device="cuda")
            assert model._device_batch_metrics(probe, (probe > 0.5).float(), torch.arange(bs * 2, device="cuda"), bs) == {}
        torch.manual_seed(0)
        best = model.fit([X[:, j] for j in range(X.shape[1])], y, batch_size=bs, epochs=2,
                         validation_data=([Xv[:, j] for j in range(X.shape[1])], yv))
        # switch on: per epoch one call over the epoch's batches and one over the validation set; off: none
        assert calls == ([bs, 0, bs, 0] if switch else [])
        vals = [h["val_auc"] for h in model.history]
        runs[switch] = (model.history, int(np.argmax(vals)), best.predict(Xv, 1024))
    capsys.readouterr()
    off, on = runs[False], runs[True]
    assert len(off[0]) == len(on[0]) == 2
    for a, b in zip(off[0], on[0]):
        assert list(a) == list(b)
        print(a, b)
        assert a["loss"] == b["loss"]
        for k in ("auc", "val_auc"):
            assert abs(a[k] - b[k]) < SKLEARN_TOL, (k, a[k], b[k])
        for k in ("acc", "val_acc"):
            assert abs(a[k] - b[k]) < 1e-12, (k, a[k], b[k])  # (a mean of three batch means, summed in another order)
    assert off[1] == on[1]                    # the same epoch wins
    assert np.array_equal(off[2], on[2])      # ... and the same model is returned


def test_cli_msl_result_row(tmp_path, monkeypatch):
    """One msl run through main with the switch in optim_config.  The result row it writes (auc_{i} masked per domain and
    total_auc from the device) equals, to the row's own four decimals, the host row of the SAME model and predictions:
    the driver's evaluate_predictions is wrapped to score them a second time with the switch off.  log_loss_{i} is the
    host's either way."""
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import main as M
    tr, te = synth_csv.make_frames(n_train=2048, n_test=1024)
    for df in (tr, te):  # two populated domains (the generator's gender column has one value) and rows of neither
        df["gender_tag"] = np.where(df["movie_tag"] % 7 == 0, 11, np.where(df["user_tag"] % 2 == 0, 5, 8))
    a, b = str(tmp_path / "train.csv"), str(tmp_path / "test.csv")
    tr.to_csv(a, index=False)
    te.to_csv(b, index=False)
    cfg = synth_csv.config(a, b, str(tmp_path / "res.csv"), "star")
    cfg["model_config"]["task_name"] = "msl"
    cfg["data_config"].update(label_columns=["label2", "label2"], num_domains=2, mask_values=[0, 1],
                              mask_column="gender_tag", scene_feature="gender_tag")
    cfg["training_config"]["epochs"] = 1
    cfg["optim_config"]["device_metrics"] = True
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg))
    original, host_rows = M.evaluate_predictions, []

    def both(model, *args):
        assert model.device_metrics is True  # (read from optim_config)
        mask = args[3]
        assert mask[:, 0].sum() > 100 and mask[:, 1].sum() > 100 and (mask.sum(1) == 0).sum() > 20
        model.device_metrics = False
        host_rows.append(original(model, *args))
        model.device_metrics = True
        return original(model, *args)

    monkeypatch.setattr(M, "evaluate_predictions", both)
    args = M.build_parser().parse_args(["--config", str(p), "--run", "1", "--model_name", "star", "--seeds", "0"])
    on = M.run(args)[0]
    off = host_rows[0]
    print(off, on)
    assert set(on) == {"type", "log_loss_0", "auc_0", "log_loss_1", "auc_1", "total_auc"}
    for k in ("auc_0", "auc_1", "total_auc"):
        assert on[k] == off[k] and 0.0 < on[k] < 1.0, (k, on[k], off[k])
    for k in ("log_loss_0", "log_loss_1"):
        assert on[k] == off[k]
