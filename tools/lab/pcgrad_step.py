#!/usr/bin/env python3
"""The PCGrad per-task step on the AE-30-shaped MMoE (B = 65 536, T = 2, one GPU), next to the "total" step, which is the
MMoE step.

  --mode time     ms per step of both, three alternating blocks each (device events around blocks of replayed steps)
  --mode profile  per_task steps only, to be run under `rocprofv3 --kernel-trace --stats` (a run of its own); also writes
                  the bytes every new kernel has to move, computed from the shapes and the batch's distinct rows
  --mode report   profiles/pcgrad_mmoe_ae30_b65536.txt from the two runs' files

tools/lab/pcgrad_step.sh runs the three in order."""
import argparse
import csv
import glob
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PEAK = 8.0e12  # bytes / s of HBM3E


def build(objectives, B, vocab_scale, table_update):
    import torch
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import workloads as W
    dev = torch.device("cuda:0")
    model, cfg, vocab, dense = W.build_model("mmoe_ae30", dev, vocab_scale=vocab_scale, seed=0, model_name="pcg",
                                             table_update=table_update)
    model.optim_config["pcgrad_objectives"] = objectives
    model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
    model.train()
    T = W.num_tasks(cfg)
    X, y = W.synth_batch(vocab, len(dense), B, T, seed=5)
    y[:, 1] = torch.where(torch.arange(B) % 4 < 3, 1.0 - y[:, 0], y[:, 1])  # conflicting tasks
    step = model.train_step_runner(B, use_graph=True)
    step.plan.X.copy_(X.to(dev))
    step.plan.y.copy_(y.to(dev))
    return model, step, X, vocab, cfg


def block_ms(step, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        step.run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def new_kernel_bytes(step, X, vocab, E):
    """Bytes each new launch has to move: banks read (and written) over the arena and the batch's distinct rows, plus the
    one mark byte per table row the marked segments look at."""
    T = step.pcgrad.T
    arena = step.store.arena.numel()
    uniq = sum(int(X[:, f].unique().numel()) for f in range(len(vocab)))
    marks = sum(vocab)
    rows = uniq * E
    return {"pcgrad_gram_kernel": 4 * T * (arena + rows) + marks,
            "pcgrad_combine_kernel": 4 * (T + 1) * (arena + rows) + marks,
            "pcgrad_stash_kernel(arena)": 8 * arena,
            "pcgrad_stash_kernel(tables)": 12 * rows + marks,
            "arena_elements": arena, "distinct_rows": uniq, "table_rows": marks, "T": T}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["time", "profile", "report"], required=True)
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--vocab-scale", type=float, default=1.0)
    ap.add_argument("--table-update", default="dense_exact")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "pcgrad_lab"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.mode == "time":
        random.seed(0)
        res = {}
        steps = {o: build(o, a.B, a.vocab_scale, a.table_update)[1] for o in ("total", "per_task")}
        for o, st in steps.items():
            for _ in range(a.warmup):
                st.run()
        for rep in range(3):
            for o, st in steps.items():
                res.setdefault(o, []).append(block_ms(st, a.steps))
        res["loss"] = {o: float(st.plan.loss.item()) for o, st in steps.items()}
        res["fired"] = steps["per_task"].pcgrad.fired.cpu().tolist()
        res["config"] = dict(B=a.B, vocab_scale=a.vocab_scale, table_update=a.table_update, steps=a.steps)
        json.dump(res, open(os.path.join(a.out, "time.json"), "w"))
        print(json.dumps(res))
    elif a.mode == "profile":
        random.seed(0)
        model, st, X, vocab, cfg = build("per_task", a.B, a.vocab_scale, a.table_update)
        for _ in range(a.warmup + a.steps):
            st.run()
        import torch
        torch.cuda.synchronize()
        json.dump(new_kernel_bytes(st, X, vocab, cfg["model_config"]["emb"]), open(os.path.join(a.out, "bytes.json"), "w"))
    else:
        t = json.load(open(os.path.join(a.out, "time.json")))
        by = json.load(open(os.path.join(a.out, "bytes.json")))
        stats = sorted(glob.glob(os.path.join(a.out, "prof", "**", "*kernel_stats.csv"), recursive=True))
        lines = ["PCGrad per-task step, AE-30-shaped MMoE, one MI355X; config " + json.dumps(t["config"]),
                 "ms per step, three alternating blocks of %d replayed steps each (device events):" % t["config"]["steps"]]
        for o in ("total", "per_task"):
            lines.append("  %-9s %s   (min %.4f)" % (o, " ".join("%.4f" % v for v in t[o]), min(t[o])))
        lines.append("  per_task / total = %.3f;  loss total %.4f  per_task %.4f;  fired %s" % (
            min(t["per_task"]) / min(t["total"]), t["loss"]["total"], t["loss"]["per_task"], t["fired"]))
        lines.append("bytes from the shapes: arena %d elements, %d distinct rows of %d table rows, T = %d" % (
            by["arena_elements"], by["distinct_rows"], by["table_rows"], by["T"]))
        lines.append("rocprofv3 --kernel-trace --stats (a run of its own), the new kernels:")
        for f in stats[:1]:
            for row in csv.DictReader(open(f)):
                if "pcgrad" not in row["Name"]:
                    continue
                name = row["Name"].split("(")[0].replace("void ", "").replace("mml::", "")
                avg = float(row["AverageNs"])
                line = "  %-34s calls %5s  avg %9.1f us  min %9.1f  max %9.1f  %5s %% of kernel time" % (
                    name, row["Calls"], avg / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3, row["Percentage"])
                key = name.split("<")[0]
                if key == "pcgrad_stash_kernel":  # (arena and table launches share the symbol: both bounds)
                    lo, hi = by["pcgrad_stash_kernel(arena)"], by["pcgrad_stash_kernel(tables)"]
                    line += "  bytes %d (arena) / %d (tables): max %.3f of 8 TB/s at the fastest launch" % (
                        lo, hi, max(lo, hi) / (float(row["MinNs"]) * 1e-9) / PEAK)
                elif key in by:
                    line += "  bytes %d: %.3f of 8 TB/s" % (by[key], by[key] / (avg * 1e-9) / PEAK)
                lines.append(line)
        txt = "\n".join(lines) + "\n"
        open(os.path.join(ROOT, "profiles", "pcgrad_mmoe_ae30_b65536.txt"), "w").write(txt)
        open(os.path.join(a.out, "pcgrad_mmoe_ae30_b65536.txt"), "w").write(txt)
        print(txt)


if __name__ == "__main__":
    main()
