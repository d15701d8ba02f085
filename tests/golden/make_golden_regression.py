#!/usr/bin/env python3
"""Golden vectors for models with regression tasks (task_types "regression", losses "mse" / "mae").  Like make_golden.py
it runs only where the unmodified reference exists; it writes reg_*.npz next to this file: arrays and the config JSON
string.  No reference text goes in.

Cases (task types / losses; optimizer trajectories over three batches):
  reg_mmoe_mtl       MMoE mtl with a dense column   [binary, regression] / [bce, mse]            Adam, Adagrad
  reg_ple            PLE                            [regression, regression] / [mse, mae]        Adam
  reg_pepnet_mtmsl   PepNet mtmsl, four gated heads [binary, binary, regression, regression]     Adagrad (+ y_pred_masked)
  reg_star_msl       STAR msl (w2 / bias2 heads)    all regression / mse                         Adam
  reg_sharedbottom   SharedBottom                   [binary, binary] / [mse, bce] (sigmoid+MSE)  Adam
  reg_mmoe_seconds   reg_mmoe_mtl with the regression label in hundreds (watch time in seconds)  Adam, Adagrad

Per case: cfg, vocab, sparse_names, dense_names, X0..X2, y0..y2, mask0 (msl / mtmsl), state/, frozen/ (STAR),
init_y_pred, y_pred, y_pred_masked, loss, grad/ (nograd/), and from a second instance with the same state turned
.double(): y_pred64, loss64, grad64/; <opt>_losses and <opt>1/, <opt>3/ (parameters after steps 1 and 3); `headroom`
(json: what the generator measured, see below).

Regression labels are continuous draws (no two equal, none equal to a prediction), so the sign in the MAE gradient is
never in doubt.  The generator asserts, prints and records in `headroom`:
  * the reference's own fp32 tensors meet the criteria of tests/test_regression_models_gpu.py against the float64 twin
    with at least 10x headroom;
  * for every MAE column and every sample of batch 0, |pred - y| exceeds 100x the fp32-vs-float64 prediction distance;
  * regression label columns hold no repeated value.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_regression.py [case names]
"""
import copy
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import (B, base_config, draw_batch, feature_columns, frozen_star_tensors,  # noqa: E402
                         ref_loss, ref_train_step)  # (puts the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from model.mmoe import MMOE  # noqa: E402  (reference)
from model.pepnet import PepNet  # noqa: E402
from model.ple import PLE  # noqa: E402
from model.sharedbottom import SharedBottom  # noqa: E402
from model.star import STAR  # noqa: E402

RTOL = 1e-4
BCE, MSE, MAE = "binary_crossentropy", "mse", "mae"


def with_losses(cfg, losses):
    cfg["optim_config"]["loss"] = list(losses)
    return cfg


def make_cases():
    cases = []
    for name, scale in (("reg_mmoe_mtl", 1.0), ("reg_mmoe_seconds", 300.0)):
        c = with_losses(base_config("mtl", "mmoe", ["click", "watch"], 8, "adam", 0.005, task_names=["ctr", "watch"],
                                    task_types=["binary", "regression"]), [BCE, MSE])
        cases.append(dict(name=name, cls=MMOE, cfg=c, vocab=[40, 30, 12, 7, 21], nd=1, opts=("adam", "adagrad"),
                          label_scale=scale))
    c = with_losses(base_config("mtl", "ple", ["l1", "l2"], 8, "adam", 0.005, task_names=["ratio", "stay"],
                                task_types=["regression", "regression"], expert_dnn_hidden_units=[32],
                                gate_dnn_hidden_units=[16], tower_dnn_hidden_units=[16]), [MSE, MAE])
    cases.append(dict(name="reg_ple", cls=PLE, cfg=c, vocab=[9, 3, 48, 64, 33], nd=0, opts=("adam",)))
    c = with_losses(base_config("mtmsl", "pepnet", ["label", "label", "label2", "label2"], 4, "adagrad", 0.01,
                                task_types=["binary", "binary", "regression", "regression"], dnn_hidden_units=[16, 16],
                                expert_dnn_hidden_units=[16, 8], gate_dnn_hidden_units=[8], tower_dnn_hidden_units=[8]),
                    [BCE, BCE, MSE, MSE])  # (narrow: the file stays under 1 MiB)
    c["data_config"].update({"num_domains": 2, "mask_values": [0, 1], "mask_column": "scene", "scene_feature": "scene"})
    cases.append(dict(name="reg_pepnet_mtmsl", cls=PepNet, cfg=c, vocab=[2, 12, 23, 48, 33, 2], nd=0, scene_last=True,
                      opts=("adagrad",)))
    c = with_losses(base_config("msl", "star", ["label", "label"], 8, "adam", 0.005,
                                task_types=["regression", "regression"]), [MSE, MSE])
    c["data_config"].update({"num_domains": 2, "mask_values": [0, 1], "mask_column": "scene", "scene_feature": "scene"})
    cases.append(dict(name="reg_star_msl", cls=STAR, cfg=c, vocab=[2, 12, 23, 48, 33, 2], nd=0, scene_last=True,
                      opts=("adam",)))
    c = with_losses(base_config("mtl", "sharedbottom", ["label2", "label3"], 8, "adam", 0.01, task_names=["ctr", "ctcvr"],
                                task_types=["binary", "binary"]), [MSE, BCE])
    cases.append(dict(name="reg_sharedbottom", cls=SharedBottom, cfg=c, vocab=[40, 21, 2, 7, 33], nd=0, opts=("adam",)))
    return cases


def regression_columns(cfg, T):
    return [t for t in range(T) if cfg["model_config"]["task_types"][t] == "regression"]


def draw(gen, case, T, task_name, D):
    """make_golden's batch, with the label columns of regression tasks redrawn as continuous values in
    (0.1, 2.1) * label_scale (a watch ratio; times label_scale: seconds) -- one draw per label, repeated over the domains
    of a label group like the binary ones."""
    X, y = draw_batch(gen, case["vocab"], case["nd"], T, task_name, D)
    reg = regression_columns(case["cfg"], T)
    scale = float(case.get("label_scale", 1.0))
    groups = {}
    for t in reg:
        key = 0 if task_name == "msl" else (t // D if task_name == "mtmsl" else t)
        if key not in groups:
            groups[key] = (0.1 + 2.0 * torch.rand(B, generator=gen)) * scale
        y[:, t] = groups[key]
    return X.float(), y.float()


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def elem_rel(a, b, floor=1e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.abs(a - b) / (RTOL * np.abs(b) + floor * max(np.abs(b).max(), 1e-30))).max()


def run_case(case):
    name, cls, cfg = case["name"], case["cls"], case["cfg"]
    cols, names, dn = feature_columns(case)
    torch.manual_seed(0)
    model = cls(cols, device="cpu", config=cfg)
    T = model.num_tasks
    D = cfg["data_config"].get("num_domains", 1)
    task_name = cfg["model_config"]["task_name"]
    losses_cfg = cfg["optim_config"]["loss"]
    gen = torch.Generator().manual_seed(1)
    batches = [draw(gen, case, T, task_name, D) for _ in range(3)]
    X0, y0 = batches[0]
    out = {"cfg": np.array(json.dumps(cfg)), "vocab": np.array(case["vocab"], dtype=np.int64),
           "sparse_names": np.array(names), "dense_names": np.array(dn)}
    for i, (X, y) in enumerate(batches):
        out[f"X{i}"], out[f"y{i}"] = X.numpy(), y.numpy()
    mask0 = None
    if task_name in ("msl", "mtmsl"):
        scene = X0[:, len(case["vocab"]) - 1]
        mask0 = torch.stack([(scene == v).float() for v in cfg["data_config"]["mask_values"]], 1)
        out["mask0"] = mask0.numpy()
    model.train()
    with torch.no_grad():
        out["init_y_pred"] = model(X0, None).numpy()
    g2 = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if p.dim() >= 2 or k.startswith("out."):
                p.copy_(torch.randn(p.shape, generator=g2) * 0.1)
        if cls is STAR:
            for mods in (model.linears, model.final_layers):
                for m in mods:
                    for w in m.specific_weights:
                        w.copy_(1.0 + torch.randn(w.shape, generator=g2) * 0.5)
                    m.shared_weight.copy_(torch.randn(m.shared_weight.shape, generator=g2) * 0.2)
    state0 = copy.deepcopy(model.state_dict())
    for k, v in state0.items():
        out[f"state/{k}"] = v.numpy().copy()
    frozen = frozen_star_tensors(model) if cls is STAR else {}
    for k, v in frozen.items():
        out[f"frozen/{k}"] = v
    model.eval()
    with torch.no_grad():
        out["y_pred"] = model(X0, None).numpy().copy()
        if mask0 is not None:
            out["y_pred_masked"] = model(X0, mask0).numpy().copy()
    model.train()
    model.compile(cfg["optim_config"]["optimizer"], losses_cfg, ["mse"])
    model.zero_grad()
    loss = ref_loss(model, model(X0, None).squeeze(), y0)
    (loss + model.get_regularization_loss() + model.aux_loss).backward()
    out["loss"] = np.array(loss.item(), dtype=np.float64)
    for k, p in model.named_parameters():
        out[(f"grad/{k}" if p.grad is not None else f"nograd/{k}")] = p.grad.numpy().copy() if p.grad is not None \
            else np.array(1)
    # ---- the same in float64 (a second instance with the same state)
    m64 = cls(cols, device="cpu", config=cfg)
    m64.load_state_dict(state0)
    if cls is STAR:  # the unregistered per-domain tensors too
        for pfx, mods in (("linears", m64.linears), ("final_layers", m64.final_layers)):
            for li, m in enumerate(mods):
                for d in range(len(m.specific_weights) - 1):
                    m.specific_weights[d].data.copy_(torch.from_numpy(frozen[f"{pfx}.{li}.specific_weights.{d}"]))
                    m.specific_biases[d].data.copy_(torch.from_numpy(frozen[f"{pfx}.{li}.specific_biases.{d}"]))
    m64 = m64.double()
    if cls is STAR:  # (.double() does not reach plain lists of tensors)
        for mods in (m64.linears, m64.final_layers):
            for m in mods:
                for lst in (m.specific_weights, m.specific_biases):
                    for d in range(len(lst) - 1):
                        lst[d].data = lst[d].data.double()
    m64.train()
    m64.compile(cfg["optim_config"]["optimizer"], losses_cfg, ["mse"])
    m64.zero_grad()
    X64, y64 = X0.double(), y0.double()
    yp64 = m64(X64, None).squeeze()
    out["y_pred64"] = yp64.detach().numpy().copy()
    loss64 = ref_loss(m64, yp64, y64)
    loss64.backward()
    out["loss64"] = np.array(loss64.item(), dtype=np.float64)
    for k, p in m64.named_parameters():
        if p.grad is not None:
            out[f"grad64/{k}"] = p.grad.numpy().copy()
    # ---- the three conditions
    # (y_pred is the eval-mode forward; these models have neither dropout nor BatchNorm, so it is the training one too)
    worst = dict(y=rel(out["y_pred"], out["y_pred64"]),
                 loss=abs(float(out["loss"]) - float(out["loss64"])) / abs(float(out["loss64"])), grad=0.0, table_elem=0.0)
    for k in [k for k in out if k.startswith("grad64/")]:
        g32 = out["grad/" + k[7:]]
        worst["grad"] = max(worst["grad"], rel(g32, out[k]))
        if k[7:].startswith("embedding_dict."):
            worst["table_elem"] = max(worst["table_elem"], elem_rel(g32, out[k]))
    print(f"{name}: fp32 vs float64 of the reference: " + ", ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    assert worst["y"] < RTOL / 10 and worst["loss"] < RTOL / 10 and worst["grad"] < RTOL / 10, worst
    assert worst["table_elem"] <= 0.1, worst
    mae_margin = float("inf")
    for t, ln in enumerate(losses_cfg):
        if ln != MAE:
            continue
        gap = np.abs(out["y_pred64"][:, t] - y0.numpy().astype(np.float64)[:, t])
        dist = np.abs(out["y_pred"][:, t].astype(np.float64) - out["y_pred64"][:, t])
        mae_margin = min(mae_margin, float((gap / np.maximum(dist, 1e-300)).min()))
    print(f"{name}: smallest |pred - y| / |pred32 - pred64| over the MAE columns: {mae_margin:.3g}")
    assert mae_margin > 100.0
    distinct = True
    for X, y in batches:
        for t in regression_columns(cfg, T):
            distinct = distinct and len(np.unique(y.numpy()[:, t])) == B
    print(f"{name}: regression labels without repeated values: {distinct}")
    assert distinct
    out["headroom"] = np.array(json.dumps(dict(worst, mae_margin=(None if mae_margin == float("inf") else mae_margin),
                                               labels_distinct=bool(distinct))))
    # ---- optimizer trajectories
    for opt in case["opts"]:
        model.load_state_dict(state0)
        model.compile(opt, losses_cfg, ["mse"])
        losses = []
        for i, (X, y) in enumerate(batches):
            losses.append(ref_train_step(model, X, y))
            if i in (0, 2):
                for k, v in model.state_dict().items():
                    out[f"{opt}{i + 1}/{k}"] = v.numpy().copy()
        out[f"{opt}_losses"] = np.array(losses, dtype=np.float64)
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{name}: {len(out)} arrays, {size / 1024:.0f} KiB, loss={out['loss']:.6f}, y_pred[0]={out['y_pred'][0]}")
    assert size < 1024 * 1024


if __name__ == "__main__":
    torch.set_num_threads(1)
    only = set(sys.argv[1:])
    for case in make_cases():
        if not only or case["name"] in only:
            run_case(case)
