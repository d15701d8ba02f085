#!/usr/bin/env python3
"""Gather / scatter kernels in isolation on the AE-30 tables: B in {65 536, 1 048 576}, Zipf and uniform
indices, HIP-event timed; prints one JSON line per case with the achieved fraction of the 8 TB/s HBM roofline
(algorithmic bytes: gather F*(4+8E), scatter F*(4+12E) per sample).

    python tools/bench_rows.py [--batches 65536,1048576] [--dists zipf,uniform] [--reps 20] [--graph]

--pooled P,T: P pooled `mean` fields of maxlen T (length mode, lengths uniform in [1, T]) on a 1e6-row table beside the
AE-30 fields.  Timed interleaved in ONE process, `--rounds` times each: (a) the pooled gather and scatter
(mml_gather_pool_fwd / mml_scatter_pool_bwd: every field in one launch), (b) the composition of the single-valued
kernels for the same result -- mml_gather_fwd over T pseudo-fields per pooled field into a [B, P*T*E] buffer and a torch
masked reduce, and the reverse for the backward --, (c) the single-valued gather and scatter on the AE-30 fields alone
(the box's rate).  One JSON line per case and kernel: algorithmic bytes (per sample and pooled field 4T index bytes +
4E n_valid row bytes + 4E output bytes for the gather; 4T + 4E dOut bytes + 8E n_valid row read-modify-write bytes for
the scatter; the AE-30 fields as above), the median and the spread (max - min) of the rounds in us, the fraction of 8 TB/s.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _graph_timer(fn, reps):
    """us per call of fn, `reps` calls captured into ONE HIP graph; returns a function that replays and times it."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g_ = torch.cuda.CUDAGraph()
    st_ = torch.cuda.Stream()
    with torch.cuda.stream(st_):
        with torch.cuda.graph(g_, stream=st_):
            for _ in range(reps):
                fn()
    g_.replay()
    torch.cuda.synchronize()

    def run():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g_.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3
    return run


def bench_pooled(args, ops, dev, tabs, grads, X_ae, B, dist, E, P, T):
    import numpy as np
    F, V = len(tabs), 1_000_000
    rng = np.random.default_rng(7)
    big, gbig = torch.randn(V, E, device=dev), torch.zeros(V, E, device=dev)
    ids = (np.minimum(rng.zipf(1.2, (B, P * T)), V - 1) if dist == "zipf" else rng.integers(0, V, (B, P * T)))
    lens = rng.integers(1, T + 1, (B, P))
    X = torch.cat([X_ae[:, :F], torch.from_numpy(ids.astype(np.float32)).to(dev),
                   torch.from_numpy(lens.astype(np.float32)).to(dev)], 1).contiguous()
    n_valid = float(lens.sum()) / B  # valid positions per sample, all pooled fields
    singles = [(f, f) for f in range(F)]
    pooled = [ops.PooledField(F + p * T, T, "mean", F, F + P * T + p) for p in range(P)]
    all_t, all_g = tabs + [big], grads + [gbig]
    out = torch.empty(B, (F + P) * E, device=dev)
    d_out = torch.randn(B, (F + P) * E, device=dev)
    # (b): pseudo-fields -- every position a single-valued field of the big table -- in slices of at most 64 fields
    pf_cols = list(range(F, F + P * T))
    slices = [pf_cols[i:i + 64] for i in range(0, P * T, 64)]
    wide = torch.empty(B, P * T * E, device=dev)
    dwide = torch.empty(B, P * T * E, device=dev)
    out_b = torch.empty(B, (F + P) * E, device=dev)
    ae_cols = list(range(F))
    pos = torch.arange(T, device=dev)

    def mask_and_div():
        ln = X[:, F + P * T:].reshape(B, P, 1)
        return (pos.reshape(1, 1, T) < ln).float(), ln + 1e-8

    def gather_b():
        ops.gather_fwd(tabs, X, ae_cols, out=out_b)  # [B, F*E] into the first columns (ldo = (F + P) * E)
        for i, sl in enumerate(slices):
            ops.gather_fwd([big] * len(sl), X, sl, out=wide[:, i * 64 * E:(i * 64 + len(sl)) * E])
        m, dv = mask_and_div()
        out_b[:, F * E:] = ((wide.view(B, P, T, E) * m.unsqueeze(3)).sum(2) / dv).reshape(B, P * E)

    def scatter_b():
        m, dv = mask_and_div()
        dwide.view(B, P, T, E).copy_((d_out[:, F * E:].reshape(B, P, 1, E) / dv.unsqueeze(3)) * m.unsqueeze(3))
        ops.scatter_bwd(grads, X, ae_cols, d_out)
        for i, sl in enumerate(slices):
            ops.scatter_bwd([gbig] * len(sl), X, sl, dwide[:, i * 64 * E:(i * 64 + len(sl)) * E])

    forms = {
        "a_gather": lambda: ops.gather_pool_fwd(all_t, X, singles, pooled, out=out),
        "a_scatter": lambda: ops.scatter_pool_bwd(all_g, X, singles, pooled, d_out),
        "b_gather": gather_b,
        "b_scatter": scatter_b,
        "c_gather": lambda: ops.gather_fwd(tabs, X, ae_cols, out=out_b),
        "c_scatter": lambda: ops.scatter_bwd(grads, X, ae_cols, d_out),
    }
    # the composition computes the same block (fp32 summation order aside)
    forms["a_gather"]()
    gather_b()
    torch.cuda.synchronize()
    assert torch.allclose(out, out_b, rtol=1e-5, atol=1e-6), float((out - out_b).abs().max())
    timers = {k: _graph_timer(fn, args.reps) for k, fn in forms.items()}
    times = {k: [] for k in forms}
    for _ in range(args.rounds):  # interleaved: every form once per round
        for k, run in timers.items():
            times[k].append(run())
    ae_g, ae_s = F * (4 + 8 * E), F * (4 + 12 * E)
    pg = P * (4 * T + 4 * E) + 4 * E * n_valid
    ps = P * (4 * T + 4 * E) + 8 * E * n_valid
    per = {"a_gather": ae_g + pg, "b_gather": ae_g + pg, "c_gather": ae_g,
           "a_scatter": ae_s + ps, "b_scatter": ae_s + ps, "c_scatter": ae_s}
    for k, ts in times.items():
        med = sorted(ts)[len(ts) // 2]
        gbs = B * per[k] / (med * 1e-6) / 1e9
        print(json.dumps({"form": k[0], "kernel": k[2:], "pooled": [P, T], "B": B, "dist": dist, "E": E,
                          "algorithmic_bytes": int(B * per[k]), "us": round(med, 1),
                          "spread_us": round(max(ts) - min(ts), 1), "rounds": len(ts),
                          "algorithmic_GBps": round(gbs, 1), "frac_of_8TBps": round(gbs / 8000, 3)}), flush=True)
    for gr in all_g:
        gr.zero_()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="65536,1048576")
    ap.add_argument("--dists", default="zipf,uniform")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workload", default="mmoe_ae30")
    ap.add_argument("--graph", action="store_true", help="time the launches replayed from ONE HIP graph (device time of "
                                                         "small launches; eager calls are host-bound below ~20 us)")
    ap.add_argument("--pooled", default=None, help="P,T: P pooled mean fields of maxlen T beside the workload's fields (always timed from ONE HIP "
                                                 "graph per form, with or without --graph)")
    ap.add_argument("--rounds", type=int, default=5, help="--pooled: interleaved repeats of every timed form")
    args = ap.parse_args()
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import ops, workloads as W
    dev = torch.device("cuda:0")
    cfg, names, vocab, dense = W.workload(args.workload)
    E = cfg["model_config"]["emb"]
    F = len(vocab)
    g = torch.Generator(device="cpu").manual_seed(0)
    tabs = [torch.randn(v, E, generator=g).to(dev) for v in vocab]
    grads = [torch.zeros(v, E, device=dev) for v in vocab]
    cols = list(range(F))
    for B in [int(b) for b in args.batches.split(",")]:
        for dist in args.dists.split(","):
            X, _ = W.synth_batch(vocab, 0, B, 2, seed=1, dist=dist)
            X = X.to(dev)
            d_out = torch.randn(B, F * E, device=dev)
            out = torch.empty(B, F * E, device=dev)
            if args.pooled:
                P, T = [int(v) for v in args.pooled.split(",")]
                bench_pooled(args, ops, dev, tabs, grads, X, B, dist, E, P, T)
                continue

            def timed(fn):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                if args.graph:
                    g_ = torch.cuda.CUDAGraph()
                    st_ = torch.cuda.Stream()
                    with torch.cuda.stream(st_):
                        with torch.cuda.graph(g_, stream=st_):
                            for _ in range(args.reps):
                                fn()
                    g_.replay()
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    g_.replay()
                    b.record()
                    torch.cuda.synchronize()
                    return a.elapsed_time(b) / args.reps
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.reps):
                    fn()
                b.record()
                torch.cuda.synchronize()
                return a.elapsed_time(b) / args.reps

            t_g = timed(lambda: ops.gather_fwd(tabs, X, cols, out=out))
            t_s = timed(lambda: ops.scatter_bwd(grads, X, cols, d_out))
            for name, t, per in (("gather", t_g, F * (4 + 8 * E)), ("scatter", t_s, F * (4 + 12 * E))):
                gbs = B * per / (t * 1e-3) / 1e9
                print(json.dumps({"kernel": name, "workload": args.workload, "B": B, "dist": dist, "us": round(t * 1e3, 1),
                                  "algorithmic_GBps": round(gbs, 1), "frac_of_8TBps": round(gbs / 8000, 3)}), flush=True)
            # keep the accumulators small in magnitude
            for gr in grads:
                gr.zero_()


if __name__ == "__main__":
    main()
