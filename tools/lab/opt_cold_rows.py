"""The dense table update of the AE-30 step alone (all 30 tables in one marked launch that also takes the deterministic
scatter's totals: opt_dense_kernel<true, 4, 2>, the launch bench.py's step ends with), timed against the share of rows whose
moments have left zero (mml_opt_tensor.warm_rows).  The warm rows of a line are those that N fresh Zipf batches of 65 536
samples touch (workloads.synth_batch's inverse CDF, alpha 1.05, drawn on the device), N = 4 / 30 / 300 / 1 000, and every
row for the last line; the first line is the launch without a map (every row updated).  Each replay marks the rows of one
more batch, as the scatter of a step does, and runs behind a 1 GiB pass that empties the caches; HIP events around the
launch, median of `reps` replays after `warm-up` ones.
usage: python tools/lab/opt_cold_rows.py [reps [warm-up [lines]]]   lines: e.g. 4,every (default 4,30,300,1000,every);
MMLREC_LIB=<library> times another build of the kernel (-DMML_OPT_COLD_CB=...) or the library of another commit;
MMLREC_OPT_COLD_COMPACT / MMLREC_OPT_RESIDENT pick the loop and its grid as they do in a training step (optimizer.cold_loop_of:
RESIDENT=0 the workgroups of each tensor, 2 the chip-sized grid halved), MMLREC_OPT_STEP_CONSTS=0 has every workgroup compute
Adam's bias terms."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import mmlrec_amd  # noqa: F401,E402
from mmlrec_amd import ops, optimizer as O, workloads as W  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 25
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
lines = (sys.argv[3] if len(sys.argv) > 3 else "4,30,300,1000,every").split(",")
dev = torch.device("cuda:0")
E, B, ALPHA = 8, 65536, 1.05
vocab = list(W.AE30_VOCAB)
order = sorted(range(len(vocab)), key=lambda f: vocab[f] * E >= (1 << 22))  # small tables first, as the step lists them
gen = torch.Generator(device=dev).manual_seed(1)


def zipf_rows(v, n):
    """n draws of synth_batch's bounded Zipf over v rows."""
    u = torch.rand(n, generator=gen, dtype=torch.float64, device=dev)
    r = ((float(v) ** (1.0 - ALPHA) - 1.0) * u + 1.0) ** (1.0 / (1.0 - ALPHA))
    return (r.floor() - 1).clamp_(0, v - 1).long()


def touched_after(batches):
    """Per table: byte map of the rows `batches` fresh batches touch (built on from the previous call's maps)."""
    global seen_batches
    for _ in range(batches - seen_batches):
        for f, v in enumerate(vocab):
            touched[f][zipf_rows(v, B)] = 1
    seen_batches = batches
    return [t.clone() for t in touched]


touched = [torch.zeros(v, dtype=torch.uint8, device=dev) for v in vocab]
seen_batches = 0
p = [torch.randn(v, E, device=dev) for v in vocab]
m = [torch.zeros(v, E, device=dev) for v in vocab]
s2 = [torch.zeros(v, E, device=dev) for v in vocab]
g = [torch.zeros(v, E, device=dev) for v in vocab]
acc = [torch.zeros(v, E, dtype=torch.int64, device=dev) for v in vocab]
marks = [torch.zeros(v, dtype=torch.uint8, device=dev) for v in vocab]
warm = [torch.zeros(v, dtype=torch.uint8, device=dev) for v in vocab]
slot = ops.amax_slots(1, dev)[0]
shift = ops.scatter_det_shift(B)
junk = torch.empty(1 << 28, dtype=torch.float32, device=dev)
knobs = O.OptKnobs.from_env()
# as in a training step the launch reads the step's constants from the buffer mml_opt_step_begin fills before it (outside the
# timed region); MMLREC_OPT_STEP_CONSTS=0: a host step, every workgroup computes them
step_dev, consts = ops.step_counter(dev) if knobs.step_consts else (None, None)
hyper = ops.make_hyper("adam", 1e-3, step=7, step_dev=step_dev, zero_grad=True, max_blocks=1 << 20,
                       cold_loop=O.cold_loop_of(knobs))
params = float(sum(vocab)) * E


def launch(with_map):
    ops.opt_step_dense([(p[f], g[f], m[f], s2[f], None, None, marks[f], (acc[f], slot, shift), warm[f] if with_map else None)
                        for f in order], hyper)


def timed(with_map, maps):
    ts = []
    for i in range(warmup + reps):
        for f, v in enumerate(vocab):
            if maps is not None:
                warm[f].copy_(maps[f])
            marks[f][zipf_rows(v, B)] = 1
        junk.add_(1.0)
        if step_dev is not None:
            ops.opt_step_begin(step_dev, hyper, consts)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch(with_map)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


rows = float(sum(vocab))
print("AE-30 tables, %d rows x %d, adam, one launch of opt_dense_kernel<true, 4, 2>; %d replays, us" % (rows, E, reps))
print("%-28s %10s %8s %8s %8s %14s" % ("warm rows", "share", "median", "min", "max", "TB/s at 24 B/p"))
med, lo, hi = timed(False, None)
print("%-28s %10s %8.1f %8.1f %8.1f %14.2f" % ("no map (every row)", "-", med, lo, hi, 24.0 * params / med / 1e6))
for name, n in [("every row", None) if x == "every" else ("%s batches" % x, int(x)) for x in lines]:
    maps = [torch.ones_like(t) for t in touched] if n is None else touched_after(n)
    share = sum(float(t.sum()) for t in maps) / rows
    med, lo, hi = timed(True, maps)
    print("%-28s %9.1f%% %8.1f %8.1f %8.1f %14.2f" % (name, 100.0 * share, med, lo, hi, 24.0 * params / med / 1e6))
