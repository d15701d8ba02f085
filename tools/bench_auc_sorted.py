#!/usr/bin/env python3
"""Timings of the device metrics path, one JSON line each:

  kernel    mml_auc_sorted alone, one column, n = 2^22 and 2^24: ms per call (device events) and the key traffic of a
            radix pass (24 bytes per key: the histogram reads the 8-byte key, the scatter reads and writes it) in GB/s
  evaluate  BaseModel.evaluate at 2^22 validation rows, two binary tasks: the device_metrics switch on against off (off is
            the host path over sklearn, unchanged), alternated inside this process
  epoch     the per-epoch train metrics of fit at batch 65 536 over 64 steps: _device_batch_metrics with the switch on
            against the host loop fit runs when it returns {}

    python tools/bench_auc_sorted.py [kernel] [evaluate] [epoch] [--reps R]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "n": len(v)}


def bench_kernel(reps):
    from mmlrec_amd import ops
    dev = torch.device("cuda:0")
    for logn in (22, 24):
        n = 1 << logn
        g = torch.Generator(device=dev).manual_seed(logn)
        pred = torch.rand(n, 1, device=dev, generator=g)
        y = (torch.rand(n, 1, device=dev, generator=g) < 0.3).float()
        for _ in range(3):
            out = ops.auc_sorted(pred, y)
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = ops.auc_sorted(pred, y)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        med = float(np.median(ms))
        print(json.dumps({"what": "mml_auc_sorted", "n": n, "cols": 1, "auc": float(out.item()), "ms": spread(ms),
                          "keys_per_s": n / med * 1e3,
                          # the four passes' key bytes over the WHOLE call's time (build and sweep included): a lower bound of
                          # the passes' own rate; the per-kernel times come from a rocprofv3 --kernel-trace --stats run
                          "radix_key_bytes": 4 * 24 * n, "radix_GBps_lower_bound": 4 * 24 * n / med * 1e-6,
                          "share_of_8TBps": 4 * 24 * n / med * 1e-6 / 8000}), flush=True)


def kuairec_model(metrics):
    from conftest import load_golden, randomize_he
    from test_models_gpu import build, load_state
    g = load_golden("mmoe_kuairec")
    model, cfg = build(g)
    load_state(model, g)
    randomize_he(model, 5)
    model.compile("adam", cfg["optim_config"]["loss"], metrics)
    return g, model


def bench_evaluate(reps):
    g, model = kuairec_model(["auc", "acc"])
    n = 1 << 22
    pool = np.concatenate([g["X0"], g["X1"], g["X2"]])
    rng = np.random.default_rng(1)
    X = np.stack([pool[rng.integers(0, len(pool), n), f] for f in range(pool.shape[1])], 1).astype(np.float32)
    y = (rng.random((n, 2)) < 0.35).astype(np.float32)
    times = {False: [], True: []}
    res = {}
    for rep in range(reps + 1):
        for switch in (False, True):
            model.device_metrics = switch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[switch] = model.evaluate(X, y, batch_size=65536)
            torch.cuda.synchronize()
            if rep:  # (the first round warms both paths up)
                times[switch].append(time.perf_counter() - t0)
    print(json.dumps({"what": "evaluate", "rows": n, "tasks": 2, "host_s": spread(times[False]),
                      "device_s": spread(times[True]), "host_over_device": float(np.median(times[False]) /
                                                                                 np.median(times[True])),
                      "host": res[False], "device": res[True]}), flush=True)


def bench_epoch(reps):
    _, model = kuairec_model(["auc", "acc"])
    dev = torch.device("cuda:0")
    bs, steps = 65536, 64
    n = bs * steps
    g = torch.Generator(device=dev).manual_seed(3)
    pred = torch.rand(n, 2, device=dev, generator=g)
    yd = (torch.rand(n, 2, device=dev, generator=g) < 0.35).float()
    perm_d = torch.randperm(n, device=dev, generator=g)
    y, perm = yd.cpu().numpy(), perm_d.cpu().numpy()

    def host():  # (fit's loop when _device_batch_metrics returns {})
        pe = pred.cpu().numpy().astype("float64")
        ye = y[perm]
        out = {}
        for name, fn in model.metrics.items():
            vals = [model._metric(fn, ye[s * bs:(s + 1) * bs], pe[s * bs:(s + 1) * bs], model.metric_cols.get(name))
                    for s in range(steps)]
            out[name] = np.sum(vals) / steps
        return out

    times = {False: [], True: []}
    res = {}
    for rep in range(reps + 1):
        for switch in (False, True):
            model.device_metrics = switch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if switch:
                res[switch] = model._device_batch_metrics(pred, yd, perm_d, bs)
            else:
                assert model._device_batch_metrics(pred, yd, perm_d, bs) == {}
                res[switch] = host()
            torch.cuda.synchronize()
            if rep:
                times[switch].append(time.perf_counter() - t0)
    print(json.dumps({"what": "epoch_metrics", "batch": bs, "steps": steps, "host_s": spread(times[False]),
                      "device_s": spread(times[True]), "host_over_device": float(np.median(times[False]) /
                                                                                 np.median(times[True])),
                      "host": {k: float(v) for k, v in res[False].items()}, "device": res[True]}), flush=True)


if __name__ == "__main__":
    import mmlrec_amd  # noqa: F401
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    args = [a for a in args if not a.isdigit()] or ["kernel", "evaluate", "epoch"]
    if "kernel" in args:
        bench_kernel(max(reps, 10))
    if "evaluate" in args:
        bench_evaluate(reps)
    if "epoch" in args:
        bench_epoch(reps)
