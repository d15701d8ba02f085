#!/usr/bin/env python3
"""Golden vectors for schemas with multi-valued (pooled) feature columns.  Like make_golden.py it runs only where the
unmodified reference exists; it writes pooled_*.npz next to this file: arrays, the config JSON string and a JSON
description of the columns.  No reference text goes in.

Per case: cfg, columns (json: single-valued, pooled and dense columns in DECLARATION order -- pooled ones after all
single-valued ones), X0..X2, y0..y2, mask0, state/, init_y_pred, dnn_input, layer/,
y_pred, y_pred_masked, loss, grad/, and from a second instance with the same state turned .double(): dnn_input64, y_pred64, grad64/.
Optimizer trajectories: parameters after EACH of the three steps for Adam and Adagrad, after steps 1 and 3 for RMSprop
and SGD (first case; the other cases keep steps 1 and 3 of Adam and Adagrad, PepNet of Adagrad alone: every file stays
under 1 MiB).

The generator asserts, and prints, that the reference's own fp32 tensors meet the criteria of
tests/test_pooled_models_gpu.py against the float64 ones with at least 10x headroom.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pooled.py [case names]
"""
import copy
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import B, base_config, ref_loss, ref_train_step  # noqa: E402  (puts the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from model.mmoe import MMOE  # noqa: E402  (reference)
from model.pepnet import PepNet  # noqa: E402
from model.sharedbottom import SharedBottom  # noqa: E402
from model.utils import DenseFeat, SparseFeat, VarLenSparseFeat, combined_dnn_input  # noqa: E402

RTOL = 1e-4
FOUR = [dict(name="h_mean", vocab=40, maxlen=6, combiner="mean", length_name=None, shared_with=None),
        dict(name="h_sum", vocab=50, maxlen=12, combiner="sum", length_name="h_sum_len", shared_with=None),
        dict(name="h_max", vocab=30, maxlen=5, combiner="max", length_name=None, shared_with=None),
        dict(name="h_item", vocab=None, maxlen=20, combiner="mean", length_name="h_item_len", shared_with="s1")]


def make_cases():
    cases = []
    c = base_config("mtl", "mmoe", ["l1", "l2"], 8, "adam", 0.005, task_names=["ctr", "ctcvr"],
                    task_types=["binary", "binary"])
    cases.append(dict(name="pooled_mmoe_mtl", cls=MMOE, cfg=c, vocab=[40, 30, 12, 7], pooled=FOUR, nd=1, full=True))
    c = base_config("mtmsl", "pepnet", ["label", "label", "label2", "label2"], 4, "adagrad", 0.01,
                    task_types=["binary"] * 4, dnn_hidden_units=[16, 16], expert_dnn_hidden_units=[16, 8],
                    gate_dnn_hidden_units=[8], tower_dnn_hidden_units=[8])  # (narrow: the file stays under 1 MiB)
    c["data_config"].update({"num_domains": 2, "mask_values": [0, 1], "mask_column": "scene",
                             "scene_feature": "scene"})
    cases.append(dict(name="pooled_pepnet_mtmsl", cls=PepNet, cfg=c, vocab=[12, 30, 23, 2], pooled=FOUR, nd=0,
                      scene_last=True, opts=("adagrad",)))  # (E = 4 and its own optimizer only: under 1 MiB)
    c = base_config("mtl", "mmoe", ["l1", "l2"], 16, "adam", 0.001, task_names=["ctr", "ctcvr"],
                    task_types=["binary", "binary"], expert_dnn_hidden_units=[32, 24])
    cases.append(dict(name="pooled_mmoe_e16", cls=MMOE, cfg=c, vocab=[40, 9, 5],
                      pooled=[dict(name="h50", vocab=60, maxlen=50, combiner="mean", length_name=None,
                                   shared_with=None)], nd=0))
    c = base_config("mtl", "sharedbottom", ["label2", "label3"], 8, "adam", 0.01, task_names=["ctr", "ctcvr"],
                    task_types=["binary", "binary"])
    cases.append(dict(name="pooled_sharedbottom_sum", cls=SharedBottom, cfg=c, vocab=[40, 21, 7],
                      pooled=[dict(name="hs", vocab=45, maxlen=9, combiner="sum", length_name=None,
                                   shared_with=None)], nd=2))
    return cases


def feature_columns(case):
    vocab, emb = case["vocab"], case["cfg"]["model_config"]["emb"]
    names = [f"s{i}" for i in range(len(vocab))]
    if case.get("scene_last"):
        names[-1] = "scene"
    cols = [SparseFeat(n, vocabulary_size=v, embedding_dim=emb) for n, v in zip(names, vocab)]
    desc = []
    for p in case["pooled"]:
        v = vocab[names.index(p["shared_with"])] if p["shared_with"] else p["vocab"]
        cols.append(VarLenSparseFeat(SparseFeat(p["name"], vocabulary_size=v, embedding_dim=emb,
                                                embedding_name=p["shared_with"] or p["name"]),
                                     maxlen=p["maxlen"], combiner=p["combiner"], length_name=p["length_name"]))
        desc.append(dict(p, vocab=v))
    dn = [f"d{j}" for j in range(case["nd"])]
    cols += [DenseFeat(n, 1) for n in dn]
    case["cfg"]["data_config"]["dense_columns"] = dn
    return cols, names, dn, desc


def zipf_ids(gen, v, shape, lo):
    """Zipf-like ids in [lo, v): sequences repeat ids inside themselves and across samples."""
    u = torch.rand(shape, generator=gen)
    return (torch.floor(v ** u - 1.0).clamp(0, v - 1 - lo) + lo).float()


def draw_batch(gen, case, desc, T, task_name, D):
    vocab = case["vocab"]
    cols = []
    for i, v in enumerate(vocab):
        idx = zipf_ids(gen, v, (B,), 0) if (i % 3 == 0 and v > 4) else torch.randint(0, v, (B,), generator=gen).float()
        cols.append(idx.reshape(B, 1))
    cols[0][0], cols[0][1] = 0.0, float(vocab[0] - 1)
    for p in desc:
        v, L = p["vocab"], p["maxlen"]
        lo_len = 1 if p["combiner"] == "max" else 0  # an all-padded max sample's gradient depends on torch's tie-breaking
        n = torch.randint(lo_len, L + 1, (B,), generator=gen)
        pos = torch.arange(L).reshape(1, L)
        if p["length_name"] is None:  # mask mode: id 0 is padding, left-packed, some with a padded slot in the middle
            ids = zipf_ids(gen, v, (B, L), 1)
            ids[pos >= n.reshape(B, 1)] = 0.0
            hole = (torch.rand(B, generator=gen) < 0.25) & (n > 2)
            ids[hole, 1] = 0.0
            ids[2, 0], ids[3, 0] = 1.0, float(v - 1)  # rows 1 and V - 1 forced to appear
            cols.append(ids)
        else:  # length mode: id 0 is an ordinary row; ids beyond the length stay in X
            ids = zipf_ids(gen, v, (B, L), 0)
            ids[2, 0], ids[3, 0] = 1.0, float(v - 1)
            n[2], n[3] = max(1, L // 2), max(1, L // 2)
            cols += [ids, n.float().reshape(B, 1)]
    X = torch.cat(cols, 1)
    if case["nd"]:
        X = torch.cat([X, torch.rand(B, case["nd"], generator=gen)], 1)
    if task_name == "mtmsl":
        a = (torch.rand(B, 1, generator=gen) < 0.4).float()
        b2 = (torch.rand(B, 1, generator=gen) < 0.3).float()
        y = torch.cat([a.repeat(1, D), b2.repeat(1, D)], 1)
    else:
        y = (torch.rand(B, T, generator=gen) < 0.4).float()
    return X.float(), y.float()


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def elem_rel(a, b, floor=1e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.abs(a - b) / (RTOL * np.abs(b) + floor * max(np.abs(b).max(), 1e-30))).max()


def dnn_input_of(model, X):
    sl, dl = model.input_from_feature_columns(X, model.dnn_feature_columns, model.embedding_dict)
    return combined_dnn_input(sl, dl)


def run_case(case):
    name, cls, cfg = case["name"], case["cls"], case["cfg"]
    cols, names, dn, desc = feature_columns(case)
    torch.manual_seed(0)
    model = cls(cols, device="cpu", config=cfg)
    T = model.num_tasks
    D = cfg["data_config"].get("num_domains", 1)
    task_name = cfg["model_config"]["task_name"]
    gen = torch.Generator().manual_seed(1)
    batches = [draw_batch(gen, case, desc, T, task_name, D) for _ in range(3)]
    X0, y0 = batches[0]
    out = {"cfg": np.array(json.dumps(cfg)), "vocab": np.array(case["vocab"], dtype=np.int64),
           "sparse_names": np.array(names), "dense_names": np.array(dn), "columns": np.array(json.dumps(desc))}
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
    state0 = copy.deepcopy(model.state_dict())
    for k, v in state0.items():
        out[f"state/{k}"] = v.numpy().copy()
    model.eval()
    model.update_save(True)
    with torch.no_grad():
        yp = model(X0, None)
        for k, v in getattr(model, "layer_output_dict", {}).items():
            out[f"layer/{k}"] = v.numpy().copy()
        out["y_pred"] = yp.numpy().copy()
        if mask0 is not None:
            out["y_pred_masked"] = model(X0, mask0).numpy().copy()
        out["dnn_input"] = dnn_input_of(model, X0).numpy().copy()
    model.update_save(False)
    model.train()
    model.compile(cfg["optim_config"]["optimizer"], cfg["optim_config"]["loss"], ["auc", "acc"])
    model.zero_grad()
    loss = ref_loss(model, model(X0, None).squeeze(), y0)
    (loss + model.get_regularization_loss() + model.aux_loss).backward()
    out["loss"] = np.array(loss.item(), dtype=np.float64)
    for k, p in model.named_parameters():
        out[(f"grad/{k}" if p.grad is not None else f"nograd/{k}")] = p.grad.numpy().copy() if p.grad is not None \
            else np.array(1)
    # ---- the same in float64
    # (a second instance with the same state: copy.deepcopy(model) fails on PepNet once a forward has left non-leaf
    # tensors on the module)
    m64 = cls(cols, device="cpu", config=cfg)
    m64.load_state_dict(state0)
    m64 = m64.double()
    m64.train()
    m64.compile(cfg["optim_config"]["optimizer"], cfg["optim_config"]["loss"], ["auc", "acc"])
    m64.zero_grad()
    X64, y64 = X0.double(), y0.double()
    with torch.no_grad():
        out["dnn_input64"] = dnn_input_of(m64, X64).numpy().copy()
    yp64 = m64(X64, None).squeeze()
    out["y_pred64"] = yp64.detach().numpy().copy()
    loss64 = ref_loss(m64, yp64, y64)
    loss64.backward()
    out["loss64"] = np.array(loss64.item(), dtype=np.float64)
    for k, p in m64.named_parameters():
        if p.grad is not None:
            out[f"grad64/{k}"] = p.grad.numpy().copy()
    # ---- the reference's own fp32 tensors against float64: the criteria hide nothing
    worst = dict(dnn=rel(out["dnn_input"], out["dnn_input64"]), y=rel(out["y_pred"], np.abs(out["y_pred64"]) * 0 + out["y_pred64"]),
                 loss=abs(float(out["loss"]) - float(out["loss64"])) / float(out["loss64"]), grad=0.0, table_elem=0.0)
    model.eval()
    for k in [k for k in out if k.startswith("grad64/")]:
        g32 = out["grad/" + k[7:]]
        worst["grad"] = max(worst["grad"], rel(g32, out[k]))
        if k[7:].startswith("embedding_dict."):
            worst["table_elem"] = max(worst["table_elem"], elem_rel(g32, out[k]))
    model.train()
    print(f"{name}: fp32 vs float64 of the reference: " + ", ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    assert worst["dnn"] < RTOL / 10 and worst["loss"] < RTOL / 10 and worst["grad"] < RTOL / 10
    assert worst["table_elem"] <= 0.1, worst
    # ---- optimizer trajectories
    opts = case.get("opts") or ("adam", "adagrad") + (("rmsprop", "sgd") if case.get("full") else ())
    for opt in opts:
        model.load_state_dict(state0)
        model.compile(opt, cfg["optim_config"]["loss"], ["auc", "acc"])
        losses = []
        for i, (X, y) in enumerate(batches):
            losses.append(ref_train_step(model, X, y))
            every = case.get("full") and opt in ("adam", "adagrad")
            if every or i in (0, 2):
                for k, v in model.state_dict().items():
                    out[f"{opt}{i + 1}/{k}"] = v.numpy().copy()
        out[f"{opt}_losses"] = np.array(losses, dtype=np.float64)
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB, loss={out['loss']:.6f}, "
          f"y_pred[0]={out['y_pred'][0]}")


if __name__ == "__main__":
    torch.set_num_threads(1)
    only = set(sys.argv[1:])
    for case in make_cases():
        if not only or case["name"] in only:
            run_case(case)
