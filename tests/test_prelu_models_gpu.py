"""dnn_activation "prelu" through BaseModel, the engine and the fused train step.

Against fixtures made from the unmodified reference (tests/golden/make_golden_prelu.py -> tests/golden/prelu_*.npz), with
the structure and the criteria of tests/test_regression_models_gpu.py: state keys and seeded init, predictions (masked
too), loss and every gradient through autograd in both GEMM arithmetics (1e-4 max-norm, slopes included; table gradients
by the element rule), and fused steps against the stored trajectories.  The BatchNorm case adds what
tests/test_models_gpu.py does for models with BatchNorm (conftest.bn_noise_keys: the bias in front of a BatchNorm has a
structurally zero gradient, noise on both sides).

Zoo rule: every class that reads dnn_activation builds with "prelu" if it builds with "linear", and then equals the
linear model at slopes 1 and the relu model at slopes 0 -- or refuses at construction and is on the documented list."""
import json

import numpy as np
import pytest
import torch

from conftest import bn_noise_keys, load_golden, randomize_he, table_update_report
from test_models_gpu import build, elem_rel, load_state, rel
from test_regression_models_gpu import touched_rows

pytestmark = pytest.mark.gpu

RTOL = 1e-4
PRELU_CASES = ["prelu_mmoe_mtl", "prelu_ple", "prelu_star_msl", "prelu_sharedbottom_bn"]
# fixtures of the classes that read dnn_activation (DNN stacks or STAR's layers) ...
ZOO = ["sharedbottom_ml", "mmoe_kuairec", "ple_ijcai", "hmoe_ml", "esmm_ml", "escm_ml", "cross_stitch_ae", "aitm_ml",
       "star_amazon"]
# ... and of those with an activation site outside DNN / STAR that refuses it ("PReLU")
REFUSING = {"snr_trans_ae": "SNR_trans", "mssm_ml": "MSSM", "apg_ae": "APG"}


def is_slope(k):
    return "activation_layers." in k


@pytest.fixture(params=PRELU_CASES)
def pcase(request):
    return request.param, load_golden(request.param)


@pytest.fixture(params=["fp16x2", "bf16x3"])
def arith(request, monkeypatch):
    """GEMM arithmetic of the recorded plans, as in tests/test_models_gpu.py."""
    monkeypatch.setenv("MMLREC_AMAX", "1" if request.param == "fp16x2" else "0")
    return request.param


def bce_sum(yp, y):
    bce = torch.nn.functional.binary_cross_entropy
    return sum(bce(yp[:, i], y[:, min(i, y.shape[1] - 1)], reduction="sum") for i in range(yp.shape[1]))


def test_fixture_state_dict_and_seeded_init(pcase):
    name, g = pcase
    model, cfg = build(g)
    want = {k[6:]: g[k].shape for k in g.files if k.startswith("state/")}
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert set(got) == set(want) and any(is_slope(k) for k in got)
    for k in want:
        assert got[k] == tuple(want[k]), k
    model.train()
    with torch.no_grad():
        y = model(torch.from_numpy(g["X0"]).cuda())
    print(f"[{name}] init_y_pred rel={rel(y.cpu().numpy(), g['init_y_pred']):.3g}")
    assert rel(y.cpu().numpy(), g["init_y_pred"]) < RTOL


def test_fixture_forward_and_mask(pcase, arith):
    name, g = pcase
    model, cfg = build(g)
    load_state(model, g)
    model.eval()
    X = torch.from_numpy(g["X0"]).cuda()
    with torch.no_grad():
        y = model(X).cpu().numpy()
    print(f"[{name} {arith}] y_pred rel={rel(y, g['y_pred64']):.3g}")
    assert rel(y, g["y_pred"]) < RTOL and rel(y, g["y_pred64"]) < RTOL
    for t in range(y.shape[1]):
        assert rel(y[:, t], g["y_pred64"][:, t]) < RTOL, t
    if "y_pred_masked" in g.files:
        with torch.no_grad():
            ym = model(X, torch.from_numpy(g["mask0"]).cuda()).cpu().numpy()
        assert rel(ym, g["y_pred_masked"]) < RTOL
    p = model.predict(g["X0"], batch_size=64)
    assert p.dtype == np.float64 and rel(p, g["y_pred"]) < RTOL


def test_fixture_autograd_gradients(pcase, arith):
    name, g = pcase
    model, cfg = build(g)
    load_state(model, g)
    model.train()
    X, y = torch.from_numpy(g["X0"]).cuda(), torch.from_numpy(g["y0"]).cuda()
    yp = model(X)
    loss = bce_sum(yp, y)
    (loss + model.get_regularization_loss().sum()).backward()
    print(f"[{name} {arith}] loss rel={abs(float(loss) - float(g['loss64'])) / float(g['loss64']):.3g}")
    assert abs(float(loss) - float(g["loss"])) / float(g["loss"]) < RTOL
    assert abs(float(loss) - float(g["loss64"])) / float(g["loss64"]) < RTOL
    noise_bias, _ = bn_noise_keys(model.state_dict().keys())
    gscale = max(float(np.abs(g[k]).max()) for k in g.files if k.startswith("grad64/"))
    slopes = 0
    for n, p in model.named_parameters():
        if "grad64/" + n in g.files:
            assert p.grad is not None, n
            if n in noise_bias:  # structurally zero gradient: rounding noise on both sides (tests/test_models_gpu.py)
                assert float(p.grad.abs().max()) < 1e-5 * gscale, n
                continue
            r = rel(p.grad.cpu().numpy(), g["grad64/" + n])
            if is_slope(n):
                slopes += 1
                print(f"[{name} {arith}] {n}: a={float(p):.4g} da={float(p.grad):.6g} ref64={float(g['grad64/' + n][0]):.6g} "
                      f"rel={r:.3g}")
            assert r < RTOL, (n, r)
            if n.startswith("embedding_dict."):
                er = elem_rel(p.grad.cpu().numpy(), g["grad64/" + n])
                print(f"[{name} {arith}] {n}: rel={r:.3g} elem_rel={er:.3g}")
                assert er <= 1.0, (n, er)
        else:
            assert "nograd/" + n in g.files, n
    assert slopes >= 2


@pytest.mark.parametrize("graph", [False, True])
def test_fixture_fused_train_steps(pcase, arith, graph):
    """Step 1 against the reference's state after its first step (update criterion of conftest.table_update_report at share
    < 2e-3; rows no batch names must not move), the three losses, step 3 inside 2.5 lr per step.  The slopes are scalars:
    table_update_report holds their one element to 5 % of the reference's update."""
    name, g = pcase
    combos = [c for c in (("adam", "dense_exact"), ("adam", "lazy_exact"), ("adagrad", "sparse_rows"))
              if f"{c[0]}_losses" in g.files]
    assert combos
    for kind, tu in combos:
        model, cfg = build(g, table_update=tu)
        load_state(model, g)
        model.optim_config["optimizer"] = kind
        model.compile(kind, cfg["optim_config"]["loss"], ["auc"])
        model.train()
        assert model.optimizer().table_update == tu
        lr = cfg["optim_config"]["lr"]
        before = {k[6:]: g[k] for k in g.files if k.startswith("state/")}
        noise_bias, noise_rm = bn_noise_keys(before.keys())
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
                if i > 0 or k in noise_bias or k.endswith("num_batches_tracked"):
                    continue  # (noise_bias: the sign of rounding noise decides a whole lr-sized step, conftest.bn_noise_keys)
                b0 = before[k] if before[k].ndim else before[k].reshape(1)
                rows = touched[k] if k in touched else np.arange(b0.shape[0])
                share, r = table_update_report(b0, got.reshape(b0.shape), ref.reshape(b0.shape), rows)
                assert share < 2e-3, (kind, tu, k, share, r)
        print(f"[{name} {arith} {kind}/{tu} graph={graph}] losses {losses} ref {list(g[f'{kind}_losses'])}")
        assert np.allclose(losses, g[f"{kind}_losses"], rtol=RTOL), (kind, tu, losses, g[f"{kind}_losses"])


# ---------------------------------------------------------------------------------------------------------------
# what is recorded
# ---------------------------------------------------------------------------------------------------------------
def prelu_launches(calls):
    from mmlrec_amd import _lib as L
    lib = L.load()
    return [(c[0].__name__, int(c[1][1]), c[1][0]) for c in calls
            if c[0] in (lib.mml_prelu_batch_fwd, lib.mml_prelu_batch_bwd)]


def recorded(g, monkeypatch, **kw):
    monkeypatch.setenv("MMLREC_AMAX", "1")
    model, cfg = build(g, **kw)
    if kw:  # (another activation: the fixture's state has keys this model lacks)
        randomize_he(model, 3)
    else:
        load_state(model, g)
    model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
    model.train()
    step = model.train_step_runner(64, use_graph=False)
    p = step.plan
    return model, p, prelu_launches(p.fwd), prelu_launches(list(p.bwd) + list(p.bwd_tail) + list(p.bwd_side))


def test_one_launch_per_depth_and_none_for_relu(monkeypatch):
    g = load_golden("prelu_mmoe_mtl")
    model, plan, fwd, bwd = recorded(g, monkeypatch)
    # experts [32, 16] x 4 and gate DNNs [16] x 2 share depth 0; depth 1 is the experts'; then the two towers
    assert [(n, k) for n, k, _ in fwd] == [("mml_prelu_batch_fwd", 6), ("mml_prelu_batch_fwd", 4), ("mml_prelu_batch_fwd", 2)]
    assert [(n, k) for n, k, _ in bwd] == [("mml_prelu_batch_bwd", 2), ("mml_prelu_batch_bwd", 4), ("mml_prelu_batch_bwd", 6)]
    # the launches publish the magnitudes of y and dz themselves: no stand-alone magnitude pass names those buffers
    ys = {int(arr[i].y) for _, k, arr in fwd for i in range(k)}
    dzs = {int(arr[i].dz) for _, k, arr in bwd for i in range(k)}
    assert all(arr[i].amax_out for _, k, arr in fwd + bwd for i in range(k))
    for c in list(plan.fwd) + list(plan.bwd):
        meta = c[-1] if isinstance(c[-1], dict) else {}
        for t, _ in meta.get("need", []):
            assert t.data_ptr() not in ys and t.data_ptr() not in dzs, meta.get("kernel")
    assert plan.tower_head is None  # (the fused tower + head launch needs a relu tower)
    relu_model, rplan, rfwd, rbwd = recorded(g, monkeypatch, dnn_activation="relu")
    assert rfwd == [] and rbwd == []
    assert not any(is_slope(k) for k in relu_model.state_dict())


def test_star_shares_one_slope_per_layer_across_domains(monkeypatch):
    g = load_golden("prelu_star_msl")
    model, plan, fwd, bwd = recorded(g, monkeypatch)
    assert [(n, k) for n, k, _ in fwd] == [("mml_prelu_batch_fwd", 2)] * 2
    assert [(n, k) for n, k, _ in bwd] == [("mml_prelu_batch_bwd", 2)] * 2
    for _, k, arr in bwd:
        assert int(arr[0].dalpha) == int(arr[1].dalpha) and int(arr[0].alpha) == int(arr[1].alpha)
        assert int(arr[0].accumulate_dalpha) == int(arr[1].accumulate_dalpha) == 0
    assert [k for k in model.state_dict() if is_slope(k)] == ["activation_layers.0.weight", "activation_layers.1.weight"]


def test_standalone_dnn_forward_uses_the_kernels():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd.model.utils import DNN
    torch.manual_seed(0)
    d = DNN(12, [8, 6], activation="prelu", init_std=0.5, device="cuda:0")
    with torch.no_grad():
        d.activation_layers[0].weight.fill_(-0.5)
    x = torch.randn(63, 12, device="cuda:0")
    y = d(x)
    y.sum().backward()
    h = x.double()
    P = {k: v.detach().double().requires_grad_(True) for k, v in d.named_parameters()}
    for l in range(2):
        h = torch.nn.functional.prelu(h @ P[f"linears.{l}.weight"].t() + P[f"linears.{l}.bias"],
                                      P[f"activation_layers.{l}.weight"])
    h.sum().backward()
    assert rel(y.detach().cpu().numpy(), h.detach().cpu().numpy()) < RTOL
    for k, p in d.named_parameters():
        assert p.grad is not None and rel(p.grad.cpu().numpy(), P[k].grad.cpu().numpy()) < RTOL, k


# ---------------------------------------------------------------------------------------------------------------
# zoo rule
# ---------------------------------------------------------------------------------------------------------------
def copy_state(src, dst):
    """Every tensor of dst from src (parameters, buffers, STAR's unregistered per-domain lists); src's slopes are left out."""
    dst.load_state_dict({k: v for k, v in src.state_dict().items() if not is_slope(k)}, strict=True)
    for pfx in ("linears", "final_layers"):
        for ms, md in zip(getattr(src, pfx, []), getattr(dst, pfx, [])):
            if hasattr(ms, "specific_weights"):
                for d in range(len(ms.specific_weights) - 1):
                    md.specific_weights[d].data.copy_(ms.specific_weights[d].data)
                    md.specific_biases[d].data.copy_(ms.specific_biases[d].data)


def outputs_and_grads(model, g):
    X, y = torch.from_numpy(g["X0"]).cuda(), torch.from_numpy(g["y0"]).cuda()
    model.eval()
    with torch.no_grad():
        pred = model(X).cpu().numpy()
    model.train()
    model.zero_grad()
    bce_sum(model(X), y).backward()
    return pred, {k: (None if p.grad is None else p.grad.cpu().numpy().copy()) for k, p in model.named_parameters()}


@pytest.mark.parametrize("name", ZOO)
def test_zoo_prelu_is_linear_at_slope_one_and_relu_at_slope_zero(name):
    g = load_golden(name)
    assert json.loads(str(g["cfg"]))["model_config"].get("dnn_use_bn", False) is False
    linear, _ = build(g, dnn_activation="linear")  # the acceptance rule's premise
    model, cfg = build(g, dnn_activation="prelu")
    randomize_he(model, 11)
    slopes = [p for k, p in model.named_parameters() if is_slope(k)]
    assert slopes, "no PReLU layer"
    for value, other in ((1.0, linear), (0.0, build(g, dnn_activation="relu")[0])):
        with torch.no_grad():
            for p in slopes:
                p.fill_(value)
        copy_state(model, other)
        pred, grads = outputs_and_grads(model, g)
        pred_o, grads_o = outputs_and_grads(other, g)
        assert rel(pred, pred_o) < RTOL, (name, value)
        live = 0
        for k, go in grads_o.items():
            if go is None:
                assert grads[k] is None, k
                continue
            if float(np.abs(go).max()) == 0.0:  # (a dead relu layer of the twin: nothing to normalise by)
                assert float(np.abs(grads[k]).max()) == 0.0, k
                continue
            live += 1
            assert rel(grads[k], go) < RTOL, (name, value, k, rel(grads[k], go))
        assert live > 4
        assert any(grads[k] is not None for k in grads if is_slope(k))


@pytest.mark.parametrize("name", sorted(REFUSING))
def test_zoo_sites_outside_dnn_refuse_prelu_at_construction(name):
    g = load_golden(name)
    build(g, dnn_activation="linear")
    with pytest.raises(NotImplementedError, match="prelu"):
        build(g, dnn_activation="prelu")
    from mmlrec_amd import model as M
    assert hasattr(M, REFUSING[name])
    import os
    import re
    doc = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    section = re.split(r"\n## [^\n]*PReLU[^\n]*\n", doc)[1].split("\n## ")[0]
    assert REFUSING[name] in section.split("Refuses it")[1].split("\n* ")[0]
