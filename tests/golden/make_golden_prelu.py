#!/usr/bin/env python3
"""Golden vectors for models with dnn_activation "prelu" (one nn.PReLU() slope per DNN layer; STAR: one per layer shared
by its domains).  Like make_golden.py it runs only where the unmodified reference exists; it writes prelu_*.npz next to
this file: arrays and the config JSON string.  No reference text goes in.

Cases (B = 64, narrow layers; optimizer trajectories over three batches):
  prelu_mmoe_mtl         MMoE with gate DNNs, one dense column, l2_reg_dnn = 1e-3 (the slopes are regularised)  Adam, Adagrad
  prelu_ple              PLE                                                                                    Adam
  prelu_star_msl         STAR msl with a mask (y_pred_masked), one slope per layer for both domains             Adam
  prelu_sharedbottom_bn  SharedBottom with dnn_use_bn (fc -> bn -> prelu)                                       Adam

Per case: cfg, vocab, sparse_names, dense_names, X0..X2, y0..y2, mask0 (msl), state/, frozen/ (STAR), init_y_pred,
y_pred (eval mode), y_pred_masked, loss (the data loss), reg_loss, grad/ (nograd/; of loss + regulariser), and from a second
instance with the same state turned .double(): y_pred64 (eval mode), loss64, reg_loss64, grad64/ (of loss64 + reg_loss64);
<opt>_losses and <opt>1/, <opt>3/ (state after steps 1 and 3); `headroom` (json: what the generator measured).

The stored state: weights at He scale, tables N(0, 0.1), slopes drawn from [-0.5, 1.5] with the first exactly 0 and the
second negative.  The generator asserts, prints and records in `headroom`:
  * the reference's own fp32 tensors meet the criteria of tests/test_prelu_models_gpu.py against the float64 twin with at
    least 10x headroom (PReLU has a kink at 0: the state's seed is redrawn until no unit sits on it);
    (the bias in front of a BatchNorm has a structurally zero gradient: noise on both sides, held below 1e-6 of the
    largest gradient instead);
  * for every slope, the data part of |da| (the gradient of the loss without the regulariser) exceeds 100x its
    fp32-vs-float64 distance.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_prelu.py [case names]
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
from model.ple import PLE  # noqa: E402
from model.sharedbottom import SharedBottom  # noqa: E402
from model.star import STAR  # noqa: E402

RTOL = 1e-4


def make_cases():
    cases = []
    c = base_config("mtl", "mmoe", ["click", "like"], 8, "adam", 0.005, task_names=["ctr", "like"],
                    task_types=["binary", "binary"], dnn_activation="prelu", l2_reg_dnn=1e-3)
    cases.append(dict(name="prelu_mmoe_mtl", cls=MMOE, cfg=c, vocab=[40, 30, 12, 7, 21], nd=1, opts=("adam", "adagrad")))
    c = base_config("mtl", "ple", ["l1", "l2"], 8, "adam", 0.005, task_names=["ctr", "cvr"],
                    task_types=["binary", "binary"], expert_dnn_hidden_units=[32], gate_dnn_hidden_units=[16],
                    tower_dnn_hidden_units=[16], dnn_activation="prelu")
    cases.append(dict(name="prelu_ple", cls=PLE, cfg=c, vocab=[9, 3, 48, 64, 33], nd=0, opts=("adam",)))
    c = base_config("msl", "star", ["label", "label"], 8, "adam", 0.005, task_types=["binary", "binary"],
                    dnn_activation="prelu")
    c["data_config"].update({"num_domains": 2, "mask_values": [0, 1], "mask_column": "scene", "scene_feature": "scene"})
    cases.append(dict(name="prelu_star_msl", cls=STAR, cfg=c, vocab=[2, 12, 23, 48, 33, 2], nd=0, scene_last=True,
                      opts=("adam",)))
    c = base_config("mtl", "sharedbottom", ["label2", "label3"], 8, "adam", 0.01, task_names=["ctr", "ctcvr"],
                    task_types=["binary", "binary"], dnn_activation="prelu", dnn_use_bn=True)
    cases.append(dict(name="prelu_sharedbottom_bn", cls=SharedBottom, cfg=c, vocab=[40, 21, 2, 7, 33], nd=0,
                      opts=("adam",)))
    return cases


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def elem_rel(a, b, floor=1e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.abs(a - b) / (RTOL * np.abs(b) + floor * max(np.abs(b).max(), 1e-30))).max()


def is_slope(k):
    return "activation_layers." in k


def randomize(model, cls, seed, live):
    """He-scale weights, N(0, 0.1) tables and head biases, slopes from [-0.5, 1.5]: of the slopes a gradient reaches
    (`live`: PLE's last level builds networks nothing reads) the first is 0 and the second negative."""
    g2 = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        slopes = []
        for k, p in model.named_parameters():
            if is_slope(k):
                if k in live:
                    slopes.append(p)
                else:
                    p.copy_(-0.5 + 2.0 * torch.rand(1, generator=g2))
            elif k.startswith("embedding_dict.") or k.startswith("out."):
                p.copy_(torch.randn(p.shape, generator=g2) * 0.1)
            elif p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g2) * (2.0 / p.shape[1]) ** 0.5)
        if cls is STAR:  # [in, out] layout; the effective weight is the product of the two factors
            for mods in (model.linears, model.final_layers):
                for m in mods:
                    for w in m.specific_weights:
                        w.copy_(1.0 + torch.randn(w.shape, generator=g2) * 0.5)
                    m.shared_weight.copy_(torch.randn(m.shared_weight.shape, generator=g2) * (2.0 / m.shared_weight.shape[0]) ** 0.5)
        assert len(slopes) >= 2
        for i, p in enumerate(slopes):
            a = -0.5 + 2.0 * torch.rand(1, generator=g2)
            if i == 0:
                a = torch.zeros(1)
            elif i == 1:
                a = -0.1 - 0.4 * torch.rand(1, generator=g2)
            p.copy_(a)


def double_twin(cls, cols, cfg, state0, frozen):
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
    return m64


def data_slope_grads(model, loss):
    ks = [(k, p) for k, p in model.named_parameters() if is_slope(k)]
    gs = torch.autograd.grad(loss, [p for _, p in ks], retain_graph=True, allow_unused=True)
    return {k: float(g.item()) for (k, _), g in zip(ks, gs) if g is not None}


def live_slopes(model, X, y):
    """Names of the slopes a gradient reaches (on a copy: a BatchNorm forward moves running statistics)."""
    return set(data_slope_grads(model, ref_loss(model, model(X, None).squeeze(), y)))


def attempt(case, seed):
    name, cls, cfg = case["name"], case["cls"], case["cfg"]
    cols, names, dn = feature_columns(case)
    torch.manual_seed(0)
    model = cls(cols, device="cpu", config=cfg)
    T = model.num_tasks
    D = cfg["data_config"].get("num_domains", 1)
    task_name = cfg["model_config"]["task_name"]
    losses_cfg = cfg["optim_config"]["loss"]
    gen = torch.Generator().manual_seed(1)
    batches = [draw_batch(gen, case["vocab"], case["nd"], T, task_name, D) for _ in range(3)]
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
    for k, p in model.named_parameters():
        if is_slope(k):
            assert p.shape == (1,) and float(p.detach()) == 0.25, k
    model.train()
    with torch.no_grad():
        out["init_y_pred"] = model(X0, None).numpy()
    model.compile(cfg["optim_config"]["optimizer"], losses_cfg, ["auc"])
    live = live_slopes(copy.deepcopy(model), X0, y0)
    randomize(model, cls, seed, live)
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
    model.load_state_dict(state0)
    model.train()
    model.compile(cfg["optim_config"]["optimizer"], losses_cfg, ["auc"])
    model.zero_grad()
    loss = ref_loss(model, model(X0, None).squeeze(), y0)
    da32 = data_slope_grads(model, loss)
    reg = model.get_regularization_loss()
    (loss + reg + model.aux_loss).backward()
    out["loss"] = np.array(loss.item(), dtype=np.float64)
    out["reg_loss"] = np.array(float(reg), dtype=np.float64)
    for k, p in model.named_parameters():
        out[(f"grad/{k}" if p.grad is not None else f"nograd/{k}")] = p.grad.numpy().copy() if p.grad is not None \
            else np.array(1)
    # ---- the same in float64 (a second instance with the same state)
    m64 = double_twin(cls, cols, cfg, state0, frozen)
    X64, y64 = X0.double(), y0.double()
    m64.eval()
    with torch.no_grad():
        out["y_pred64"] = m64(X64, None).numpy().copy()
    m64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in state0.items()})
    m64.train()
    m64.compile(cfg["optim_config"]["optimizer"], losses_cfg, ["auc"])
    m64.zero_grad()
    loss64 = ref_loss(m64, m64(X64, None).squeeze(), y64)
    da64 = data_slope_grads(m64, loss64)
    reg64 = m64.get_regularization_loss()
    (loss64 + reg64 + m64.aux_loss).backward()
    out["loss64"] = np.array(loss64.item(), dtype=np.float64)
    out["reg_loss64"] = np.array(float(reg64), dtype=np.float64)
    for k, p in m64.named_parameters():
        if p.grad is not None:
            out[f"grad64/{k}"] = p.grad.numpy().copy()
    # ---- the conditions
    worst = dict(y=rel(out["y_pred"], out["y_pred64"]),
                 loss=abs(float(out["loss"]) - float(out["loss64"])) / abs(float(out["loss64"])), grad=0.0, table_elem=0.0)
    # the bias of a Linear in front of a BatchNorm has a structurally ZERO gradient (tests/conftest.py bn_noise_keys): both
    # sides hold rounding noise, held to a tenth of the 1e-5 of the largest gradient tests/test_models_gpu.py allows
    keys = {k[6:] for k in out if k.startswith("state/")}
    noise = {k for k in keys if ".linears." in k and k.endswith(".bias")
             and k.replace(".linears.", ".bn.").replace(".bias", ".weight") in keys}
    gscale = max(float(np.abs(out[k]).max()) for k in out if k.startswith("grad/"))
    for k in [k for k in out if k.startswith("grad64/")]:
        g32 = out["grad/" + k[7:]]
        if k[7:] in noise:
            assert float(np.abs(g32).max()) < 1e-6 * gscale and float(np.abs(out[k]).max()) < 1e-6 * gscale, k
            continue
        worst["grad"] = max(worst["grad"], rel(g32, out[k]))
        if k[7:].startswith("embedding_dict."):
            worst["table_elem"] = max(worst["table_elem"], elem_rel(g32, out[k]))
    slope_margin = min(abs(da64[k]) / max(abs(da32[k] - da64[k]), 1e-300) for k in da64)
    slopes = {k[6:]: float(v[0]) for k, v in out.items() if k.startswith("state/") and is_slope(k)}
    ok = (worst["y"] < RTOL / 10 and worst["loss"] < RTOL / 10 and worst["grad"] < RTOL / 10 and
          worst["table_elem"] <= 0.1 and slope_margin > 100.0)
    print(f"{name} (state seed {seed}): fp32 vs float64 of the reference: " +
          ", ".join(f"{k}={v:.3g}" for k, v in worst.items()) +
          f"; smallest |da_data| / |da32 - da64| over {len(da64)} slopes: {slope_margin:.3g}" + ("" if ok else "  -> redraw"))
    if not ok:
        return None
    vals = list(slopes.values())
    assert any(v == 0.0 for v in vals) and any(v < 0.0 for v in vals) and all(-0.5 <= v <= 1.5 for v in vals), slopes
    out["headroom"] = np.array(json.dumps(dict(worst, slope_margin=slope_margin, state_seed=seed, slopes=slopes,
                                               da_data64=da64)))
    # ---- optimizer trajectories
    for opt in case["opts"]:
        model.load_state_dict(state0)
        model.compile(opt, losses_cfg, ["auc"])
        losses = []
        for i, (X, y) in enumerate(batches):
            losses.append(ref_train_step(model, X, y))
            if i in (0, 2):
                for k, v in model.state_dict().items():
                    out[f"{opt}{i + 1}/{k}"] = v.numpy().copy()
        out[f"{opt}_losses"] = np.array(losses, dtype=np.float64)
    return out


def run_case(case):
    for seed in range(2, 40):
        out = attempt(case, seed)
        if out is not None:
            break
    else:
        raise SystemExit(f"{case['name']}: no state seed met the conditions")
    path = os.path.join(HERE, f"{case['name']}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{case['name']}: {len(out)} arrays, {size / 1024:.0f} KiB, loss={out['loss']:.6f}, y_pred[0]={out['y_pred'][0]}")
    assert size < 1024 * 1024


if __name__ == "__main__":
    torch.set_num_threads(1)
    only = set(sys.argv[1:])
    for case in make_cases():
        if not only or case["name"] in only:
            run_case(case)
