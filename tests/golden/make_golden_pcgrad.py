#!/usr/bin/env python3
"""Golden vectors for model_name "pcg": the reference's MMOE trained through its PCGrad wrapper (model/optimizer.py:10-138)
fed the list its docstring asks for, `optim.pc_backward([loss_0, ..., loss_{T-1}])`, loss_t = task t's summed BCE term.
Like make_golden_prelu.py it runs only where the unmodified reference exists; it writes pcg_*.npz next to this file: arrays
and the config JSON string.  No reference text goes in.

Cases (B = 64, narrow layers, zero regularisation, three batches, PCGrad(Adam) and PCGrad(Adagrad)):
  pcg_mmoe_mtl   T = 2; task 1's labels are the complement of task 0's on three quarters of the batch
  pcg_mmoe_t3    T = 3; task 1 as above, task 2 the complement of task 1 on half of it: the order of the projections matters

Per case: cfg, vocab, sparse_names, dense_names, X0..X2, y0..y2, state/, seed (the argument of random.seed() in front of each
trajectory), and from the PCGrad(Adam) trajectory, per step s = 0..2:
  task_losses[s, t]   the objectives;  orders[s, i, :] the order in which g_i met the g_j;  dots[s, i, q] the
  <pc_i, g_orders[s,i,q]> the class compared (fp32);  fired[s, i, j] = 1 where it projected g_i on g_j;
of step 0 also gtask/<t>/<param> (objective t's gradient), has/<param> ([T]: 1 where p.grad was not None -- 1 throughout: the
objectives are column slices of one concatenated prediction, so autograd hands every parameter a gradient, of zeros where
the task does not reach it, and the wrapper's merge is the mean everywhere), grad/<param> (the merged gradient the wrapper
hands to the optimizer); adam1/, adam3/, adagrad3/ (state_dict after steps 1 and 3);
`headroom` (json: what the generator measured).

The generator asserts, prints and records in `headroom`:
  * in every step of both trajectories at least one projection fires and at least one compared pair does not;
  * every compared |d| / (||pc_i|| ||g_j||) >= 1e-2: fp32 and double agree on every sign (the port runs the recursion on the
    Gram matrix of the ORIGINAL gradients in double, tests/test_pcgrad_cpu.py restates the loop in float64);
  * the reference's own fp32 merged gradients meet the criteria of tests/test_pcgrad_models_gpu.py (rel < 1e-4 per tensor,
    elem_rel <= 1 for tables) against a float64 twin of the class written here (`project64`), fed the same fp32 per-task
    gradients.  Measured (both cases, every step of both trajectories): worst rel 1.7e-7 (bound 1e-4), worst table
    elem_rel 4.9e-3 (bound 1); the smallest compared |d| / (||pc_i|| ||g_j||) is 2.9e-2 (T = 2) and 1.1e-2 (T = 3).  The
    state's seed is redrawn until all of the above holds (T = 2: seed 2, T = 3: seed 49).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pcgrad.py [case names]
"""
import copy
import json
import os
import random
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import B, base_config, draw_batch, feature_columns  # noqa: E402  (puts the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from model.mmoe import MMOE  # noqa: E402  (reference)

RTOL = 1e-4
SEED = 7  # random.seed() in front of each trajectory


def make_cases():
    cases = []
    c = base_config("mtl", "pcg", ["click", "like"], 8, "adam", 0.005, task_names=["ctr", "like"],
                    task_types=["binary", "binary"])
    cases.append(dict(name="pcg_mmoe_mtl", cfg=c, vocab=[40, 30, 12, 7, 21], nd=1))
    c = base_config("mtl", "pcg", ["click", "like", "buy"], 8, "adam", 0.005, task_names=["ctr", "like", "buy"],
                    task_types=["binary", "binary", "binary"])
    cases.append(dict(name="pcg_mmoe_t3", cfg=c, vocab=[33, 9, 48, 5, 21], nd=0))
    return cases


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def elem_rel(a, b, floor=1e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.abs(a - b) / (RTOL * np.abs(b) + floor * max(np.abs(b).max(), 1e-30))).max()


def conflicting_labels(y):
    """Task 1 = the complement of task 0 on the first three quarters of the batch; task 2 (if any) = the complement of
    task 1 on the first half."""
    y = y.clone()
    n = y.shape[0]
    y[:3 * n // 4, 1] = 1.0 - y[:3 * n // 4, 0]
    if y.shape[1] > 2:
        y[:n // 2, 2] = 1.0 - y[:n // 2, 1]
    return y


def randomize(model, seed):
    g2 = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.startswith("embedding_dict.") or k.startswith("out."):
                p.copy_(torch.randn(p.shape, generator=g2) * 0.1)
            elif p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g2) * (2.0 / p.shape[1]) ** 0.5)


def project64(g, has, orders):
    """The wrapper's projection and merge in float64 (this file's own statement of model/optimizer.py:47-67): g [T, n]
    the per-objective flattened gradients, has [T, n] 0 / 1, orders [T][T].  Returns (merged [n], dots [T, T] by position,
    fired [T, T] by (i, j))."""
    T = g.shape[0]
    pc = g.copy()
    dots, fired = np.zeros((T, T)), np.zeros((T, T), dtype=np.int32)
    for i in range(T):
        for q, j in enumerate(orders[i]):
            d = float(pc[i] @ g[j])
            dots[i, q] = d
            if d < 0:
                pc[i] = pc[i] - d * g[j] / float(g[j] @ g[j])
                fired[i, j] = 1
    shared = has.prod(0).astype(bool)
    merged = np.where(shared, pc.mean(0), pc.sum(0))
    return merged, dots, fired


def pc_step(model, X, y, keep=None):
    """One step of the reference's loop with the list of per-task objectives (basemodel.py:268-313, :310 given the list),
    spying on the wrapper: the order of the g_j, every compared dot product, the norms, the per-task gradients."""
    optim = model.optim
    y_pred = model(X, None).squeeze()
    optim.zero_grad()
    objs = [model.loss_func[t](y_pred[:, t], y[:, t], reduction="sum") for t in range(model.num_tasks)]
    rec = {}
    inner = optim._project_conflicting

    def spy(grads, has_grads, shapes=None):
        T = len(grads)
        ids = {g.data_ptr(): t for t, g in enumerate(grads)}
        rec["g"] = np.stack([g.numpy().copy() for g in grads])
        rec["has"] = np.stack([h.numpy().copy() for h in has_grads])
        seq = []
        dot = torch.dot

        def spy_dot(a, b):
            d = dot(a, b)
            seq.append((ids[b.data_ptr()], float(d), float(a.norm()), float(b.norm())))
            return d
        torch.dot = spy_dot
        try:
            merged = inner(grads, has_grads)
        finally:
            torch.dot = dot
        assert len(seq) == T * T
        rec["orders"] = np.array([[seq[i * T + q][0] for q in range(T)] for i in range(T)], dtype=np.int32)
        rec["dots"] = np.array([[seq[i * T + q][1] for q in range(T)] for i in range(T)], dtype=np.float64)
        rec["cos"] = np.array([[abs(seq[i * T + q][1]) / max(seq[i * T + q][2] * seq[i * T + q][3], 1e-300)
                                for q in range(T)] for i in range(T)])
        rec["merged"] = merged.numpy().copy()
        return merged
    optim._project_conflicting = spy
    try:
        optim.pc_backward(objs)
    finally:
        del optim._project_conflicting
    optim.step()
    rec["task_losses"] = np.array([float(o.item()) for o in objs], dtype=np.float64)
    return rec


def attempt(case, seed):
    name, cfg = case["name"], case["cfg"]
    cols, names, dn = feature_columns(case)
    torch.manual_seed(0)
    model = MMOE(cols, device="cpu", config=cfg)
    T = model.num_tasks
    gen = torch.Generator().manual_seed(1)
    batches = [draw_batch(gen, case["vocab"], case["nd"], T, "mtl", 1) for _ in range(3)]
    batches = [(X, conflicting_labels(y)) for X, y in batches]
    out = {"cfg": np.array(json.dumps(cfg)), "vocab": np.array(case["vocab"], dtype=np.int64),
           "sparse_names": np.array(names), "dense_names": np.array(dn), "seed": np.array(SEED)}
    for i, (X, y) in enumerate(batches):
        out[f"X{i}"], out[f"y{i}"] = X.numpy(), y.numpy()
    model.train()
    randomize(model, seed)
    state0 = copy.deepcopy(model.state_dict())
    for k, v in state0.items():
        out[f"state/{k}"] = v.numpy().copy()
    pnames = [k for k, _ in model.named_parameters()]
    sizes = [p.numel() for _, p in model.named_parameters()]
    shapes = [tuple(p.shape) for _, p in model.named_parameters()]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    worst = dict(rel=0.0, table_elem=0.0, min_cos=1.0)
    for opt in ("adam", "adagrad"):
        model.load_state_dict(state0)
        model.compile(opt, cfg["optim_config"]["loss"], ["auc"])
        assert type(model.optim).__name__ == "PCGrad"
        random.seed(SEED)
        steps = []
        for s, (X, y) in enumerate(batches):
            r = pc_step(model, X, y)
            steps.append(r)
            merged64, dots64, fired64 = project64(r["g"].astype(np.float64), r["has"].astype(np.float64),
                                                  r["orders"].tolist())
            r["fired"] = fired64
            # the class's own fp32 decisions are the float64 ones
            fired32 = np.zeros((T, T), dtype=np.int32)
            for i in range(T):
                for q in range(T):
                    if r["dots"][i, q] < 0:
                        fired32[i, r["orders"][i, q]] = 1
            if not (fired32 == fired64).all():
                print(f"{name} (state seed {seed}) {opt} step {s}: fp32 and float64 disagree on a sign  -> redraw")
                return None
            n_fired = int(fired64.sum())
            worst["min_cos"] = min(worst["min_cos"], float(r["cos"].min()))
            if n_fired == 0 or n_fired == T * T or r["cos"].min() < 1e-2:
                print(f"{name} (state seed {seed}) {opt} step {s}: fired {n_fired} of {T * T}, smallest "
                      f"|d| / (|pc_i| |g_j|) = {r['cos'].min():.3g}  -> redraw")
                return None
            for k, a, b in zip(pnames, offs[:-1], offs[1:]):
                worst["rel"] = max(worst["rel"], rel(r["merged"][a:b], merged64[a:b]))
                if k.startswith("embedding_dict."):
                    worst["table_elem"] = max(worst["table_elem"], elem_rel(r["merged"][a:b], merged64[a:b]))
            if s in (0, 2):
                for k, v in model.state_dict().items():
                    if opt == "adam" or s == 2:
                        out[f"{opt}{s + 1}/{k}"] = v.numpy().copy()
        out[f"{opt}_losses"] = np.array([r["task_losses"].sum() for r in steps], dtype=np.float64)
        if opt == "adam":
            out["task_losses"] = np.stack([r["task_losses"] for r in steps])
            out["orders"] = np.stack([r["orders"] for r in steps])
            out["dots"] = np.stack([r["dots"] for r in steps])
            out["fired"] = np.stack([r["fired"] for r in steps])
            r0 = steps[0]
            for k, a, b, shp in zip(pnames, offs[:-1], offs[1:], shapes):
                out[f"grad/{k}"] = r0["merged"][a:b].reshape(shp).copy()
                out[f"has/{k}"] = r0["has"][:, a].astype(np.int32)
                for t in range(T):
                    out[f"gtask/{t}/{k}"] = r0["g"][t, a:b].reshape(shp).copy()
        else:  # (the orders come from `random` alone: both trajectories draw the same)
            assert all((out["orders"][s] == steps[s]["orders"]).all() for s in range(3))
    ok = worst["rel"] < RTOL / 10 and worst["table_elem"] <= 0.1
    print(f"{name} (state seed {seed}): fp32 merge of the reference vs the float64 twin: rel={worst['rel']:.3g}, "
          f"table elem_rel={worst['table_elem']:.3g}; smallest |d| / (|pc_i| |g_j|) = {worst['min_cos']:.3g}; "
          f"fired per step {[int(f.sum()) for f in out['fired']]} of {T * T}" + ("" if ok else "  -> redraw"))
    if not ok:
        return None
    out["headroom"] = np.array(json.dumps(dict(worst, state_seed=seed)))
    return out


def run_case(case):
    for seed in range(2, 60):
        out = attempt(case, seed)
        if out is not None:
            break
    else:
        raise SystemExit(f"{case['name']}: no state seed met the conditions")
    path = os.path.join(HERE, f"{case['name']}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{case['name']}: {len(out)} arrays, {size / 1024:.0f} KiB, orders of step 0: {out['orders'][0].tolist()}")
    assert size < 1024 * 1024


if __name__ == "__main__":
    torch.set_num_threads(1)
    only = set(sys.argv[1:])
    for case in make_cases():
        if not only or case["name"] in only:
            run_case(case)
