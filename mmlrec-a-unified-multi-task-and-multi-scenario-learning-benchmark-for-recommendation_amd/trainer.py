"""One fused training step = forward launches + head/BCE launch + backward launches + optimizer launches, recorded
once per batch size and replayed (as HIP graphs when enabled).  Counterpart of the loop body of BaseModel.fit in the
reference (model/basemodel.py:261-313) minus logging.

Default (round 5): ONE HIP stream, the whole step one HIP graph (resolve_overlap below holds the A/B).  With two streams
(overlap=True / MMLREC_STREAMS=2), after the backward chain has produced every dL/d(pre-activation), the step forks --
  main stream : table scatter -> table optimizer            (HBM / atomics bound)
  side stream : all weight-gradient GEMMs -> [all-reduce] -> MLP optimizer   (MFMA bound)
-- and joins at the end: the table stream of the reference-exact dense Adam beside the wgrad GEMMs.

Multi-GPU steps (parallel.py) contain Python-issued entries (collectives, the row-sharded exchange with its run-time
sizes).  Those run eagerly; the runs of C-ABI calls between them -- static shapes, static pointers -- are still captured
and replayed as HIP graphs (`Segments`).

How a step is put together: StepKnobs.from_env reads every MMLREC_* switch once per TrainStep; whole_step_calls (one
list, with or without a fork / join inside it) and segmented_step (the two-stream lists, early fork and split dense table
update included) are pure functions of call lists; OneList, TwoStreams and PCGradSchedule replay what they return and
own their streams and events.  TrainStep picks the schedule and keeps the lists readable under their names.
"""
import dataclasses
import os
import typing

import torch

from . import engine as E
from . import passes
from .ops import concurrent_stream as ops_concurrent_stream
from . import profiling


@dataclasses.dataclass(frozen=True)
class StepKnobs:
    """Every environment switch the trainer reads, read ONCE per TrainStep (from_env; never at import: tests and lab scripts
    set the variables between constructions)."""
    streams: int = 1             # MMLREC_STREAMS=2: two streams where the caller leaves overlap=None (resolve_overlap)
    grad_marks: bool = True      # MMLREC_GRAD_MARKS=0 or MMLREC_SCATTER_OLD: the dense update reads every row's gradient
    merge_reduces: bool = True   # MMLREC_MERGE_REDUCES=0: the head / gate reductions stay where they were recorded
    merge_wgrad: bool = True     # MMLREC_MERGE_WGRAD=0: one weight-gradient launch per layer
    # CU partition of the forked tail (lab knob MMLREC_CU_TAIL = n: table scatter + table optimizer on compute units
    # [0, n), weight-gradient GEMMs + MLP optimizer on [n, all)); MMLREC_CU_EARLY = n: the early table pass on [0, n)
    cu_tail: int = 0
    cu_early: int = 0
    # The weight gradients on a second stream INSIDE the step's one graph (a fork / join of graph nodes: no seam): beside
    # the table scatter and the table optimizer.  Same-box interleaved pairs (tools/lab/ab_env.sh MMLREC_INNER_FORK=0 / 2,
    # B = 65 536): AE-30 1.4773 / 1.4818 / 1.4860 / 1.4952 / 1.4772 -> 1.4635 / 1.4683 / 1.4851 / 1.4623 / 1.4731 ms,
    # AE-30d 1.613 -> 1.582, PLE 1.535 -> 1.509, PepNet 2.028 -> 2.006; at B = 4 096 it loses (0.670 -> 0.679 ms), so
    # large batches only.  MMLREC_INNER_FORK: 0 off, 1 joined in front of the table optimizer (beside the scatter only:
    # level), 2 joined behind it (the default form), 3 forked behind the scatter; unset (None) = by batch size.
    # Round 6: the fork makes the step's graph a multi-branch graph, the kind whose launch segfaulted sporadically in
    # this runtime (hip::Graph::UpdateStreams, see TwoStreams: dependent on how many streams the process created).
    # Soaked (tools/lab/fork_soak.sh, profiles/r06_fork_soak.txt): 0 crashes in 32 fresh processes with the fork forced
    # on for EVERY batch size (22 runs of the suite's graph tests -- every model of the zoo, its own streams, the original
    # repro's shape -- and 10 of bench.py), so it stays the default for large batches; it never applies to a step that
    # holds a collective (Python-issued entries between fork and join), i.e. to no multi-GPU step.
    inner_fork: typing.Optional[int] = None
    fork_mlp: bool = False       # MMLREC_FORK_MLP=1: the MLP optimizer behind the weight gradients on the fork's branch
    early_wgrad: str = "0"       # MMLREC_EARLY_WGRAD: "0" off, "auto", or an index into plan.bwd (_early_fork)
    early_wgrad_debug: bool = False  # MMLREC_EARLY_WGRAD_DEBUG: _early_fork prints its estimate

    @staticmethod
    def streams_from_env(env=None):
        """MMLREC_STREAMS alone (resolve_overlap: on the per-batch path of fit(), which needs no other knob)."""
        return 2 if (os.environ if env is None else env).get("MMLREC_STREAMS", "1") == "2" else 1

    @classmethod
    def from_env(cls, env=None):
        env = os.environ if env is None else env
        fork = env.get("MMLREC_INNER_FORK")
        return cls(streams=cls.streams_from_env(env),
                   grad_marks=env.get("MMLREC_GRAD_MARKS", "1") != "0" and not env.get("MMLREC_SCATTER_OLD"),
                   merge_reduces=env.get("MMLREC_MERGE_REDUCES", "1") != "0",
                   merge_wgrad=env.get("MMLREC_MERGE_WGRAD", "1") != "0",
                   cu_tail=int(env.get("MMLREC_CU_TAIL", "0")), cu_early=int(env.get("MMLREC_CU_EARLY", "0")),
                   inner_fork=int(fork) if fork is not None else None,
                   fork_mlp=env.get("MMLREC_FORK_MLP", "0") == "1",
                   early_wgrad=env.get("MMLREC_EARLY_WGRAD", "0"),
                   early_wgrad_debug=bool(env.get("MMLREC_EARLY_WGRAD_DEBUG")))

    def fork_placement(self, B):
        """Where the one-list step forks (whole_step_calls): the knob, else 2 from a batch of 16 384 on and 0 below."""
        return self.inner_fork if self.inner_fork is not None else (2 if int(B) >= 16384 else 0)


class Segments:
    """A call list cut at its Python-issued entries: [graphable run, PY entry, graphable run, ...]."""

    def __init__(self, calls, use_graph, min_calls=2):
        self.parts = []  # ("c", [calls]) | ("py", call)
        run = []
        for c in calls:
            if c[0] is E.PY:
                if run:
                    self.parts.append(["c", run, None])
                    run = []
                self.parts.append(["py", c, None])
            else:
                run.append(c)
        if run:
            self.parts.append(["c", run, None])
        self.use_graph = bool(use_graph)
        self.min_calls = min_calls
        self.captured = False

    def capture(self):
        """Record every long-enough run as its own single-stream HIP graph (nothing executes)."""
        if not self.use_graph or self.captured:
            return
        for p in self.parts:
            if p[0] == "c" and len(p[1]) >= self.min_calls:
                g = torch.cuda.CUDAGraph()
                # thread_local: only THIS thread's calls are checked during capture.  In the default global mode an
                # event query of RCCL's watchdog thread (it polls while a process group exists) is an illegal call
                # during capture: it invalidates the capture or aborts the process at teardown (seen as a sporadic
                # "Fatal Python error: Aborted" in destroy_process_group).
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    E.Plan._run(p[1])
                p[2] = g
        self.captured = True

    def run(self, skip_py=None):
        for kind, item, graph in self.parts:
            if kind == "py":
                if skip_py is not None and skip_py(item):
                    continue
                item[1](*item[2])
            elif graph is not None:
                if profiling.enabled:
                    with profiling.range("hip_graph[%d calls: %s ...]" % (
                            len(item), E.call_meta(item[0]).get("kernel", getattr(item[0][0], "__name__", "inline")))):
                        graph.replay()
                else:
                    graph.replay()
            else:
                E.Plan._run(item)

    @property
    def n_graphs(self):
        return sum(1 for p in self.parts if p[2] is not None)


def fork_conflicts(side_calls, mid_calls, shared_scratch=()):
    """Raw device pointers that make a fork of `side_calls` beside `mid_calls` unsafe, as far as the call lists show it:
    (a) a shared scratch buffer (ops.workspace: every non-deferred row kernel writes its partial sums there) named by
    EITHER branch -- the other branch, or the chain that follows, may overwrite it -- and (b) a pointer argument both
    branches carry (each branch must own what it names; descriptors hold further pointers the lists do not show: the
    operands of the weight-gradient GEMMs are written by the chain BEFORE the fork and only read after it).  Returns the
    offending pointers (empty = no conflict seen); whole_step_calls refuses to fork on any (tests/test_plan_passes_cpu.py)."""
    def ptrs(calls):
        out = set()
        for c in calls:
            if c[0] is E.PY or c[0] is E.INLINE:
                continue
            for a in c[1]:
                # (device addresses on this platform are 47-bit values far above 2^32; sizes, pitches and counts -- a
                # batch of 65 536 rows is 0x10000 in BOTH lists -- stay below)
                if isinstance(a, int) and not isinstance(a, bool) and a >= (1 << 32):
                    out.add(a)
            # (buffers a call reads or writes through its descriptors and names in its meta: the 64-bit totals and the
            # magnitude slot the deterministic scatter hands to the table optimizer)
            out.update(int(p) for p in E.call_meta(c).get("ptrs", ()))
        return out
    a, b = ptrs(side_calls), ptrs(mid_calls)
    scratch = {int(x) for x in shared_scratch if x}
    return sorted(((a | b) & scratch) | (a & b))


class InnerFork:
    """A fork / join INSIDE one call list (one HIP graph): `fork` sends `calls` to a second stream behind everything
    issued so far, `join` makes the current stream wait for them.  Knob MMLREC_INNER_FORK (StepKnobs): no graph seam,
    unlike the two-stream schedule of overlap=True -- but a multi-branch graph (see TwoStreams' note on
    hip::Graph::UpdateStreams and the soak of round 6)."""

    def __init__(self, device, calls):
        self.side = torch.cuda.Stream(device=device)
        self.calls = calls
        self.ev_fork, self.ev_join = torch.cuda.Event(), torch.cuda.Event()

    def fork(self):
        self.ev_fork.record(torch.cuda.current_stream())
        self.side.wait_event(self.ev_fork)
        with torch.cuda.stream(self.side):
            E.Plan._run(self.calls)
            self.ev_join.record(self.side)

    def join(self):
        torch.cuda.current_stream().wait_event(self.ev_join)


def _quiesce_collective_watchdog():
    """Called after a device-wide synchronize and before a HIP-graph capture.  While an RCCL process group exists, its
    watchdog thread polls the end events of the collectives it has not seen complete yet (every ~100 ms).  A poll that
    lands inside a capture is an event query during stream capture: with capture_error_mode="thread_local" (Segments)
    it no longer invalidates the capture, but it was still seen -- 1 run in 24 of the suite's graph tests, round 6 -- as an
    exception in the watchdog that surfaces as "Fatal Python error: Aborted" in the NEXT destroy_process_group.  Every
    collective issued so far HAS completed (the synchronize above); giving the watchdog two of its periods to notice
    leaves it nothing to query while the capture runs.  Once per TrainStep (captures happen on the second call of run())."""
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_backend() == "nccl":
            import time
            time.sleep(0.25)
    except Exception:  # (never cost a step for this)
        pass


def resolve_overlap(overlap):
    """Stream schedule of a fused step: None = the default.  Round 5: ONE stream -- the whole step as one HIP graph.
    Same-box interleaved A/B of bench.py (three pairs each, tools/lab/ab_streams.sh, profiles/r05_ab_streams.txt): the
    forked tail (table scatter + table optimizer | weight-gradient GEMMs + MLP optimizer on a second stream) returned
    +0.5 % on AE-30 at B = 65 536 (1.7158 against 1.7265 ms) and LOST 3.4 % at B = 4 096 (0.693 against 0.670), 1.8 % on
    PepNet / Amazon-8 (2.238 against 2.200), level on KuaiRec-32: everything it co-schedules is HBM-bound together, and
    every graph seam costs ~16 us of idle stream.  Two streams stay available: overlap=True, or MMLREC_STREAMS=2."""
    if overlap is None:
        return StepKnobs.streams_from_env() == 2
    return bool(overlap)


def draw_pcgrad_orders(T):
    """The orders in which PCGrad projects: the reference shuffles ONE list of the T gradients in place before every g_i
    (model/optimizer.py:50-51: `random.shuffle(grads)` inside the loop over pc_grad), so the shuffles accumulate from one i
    to the next, and the list starts in task order at every step (_pack_grad builds it anew).  Same calls to Python's
    `random` in the same sequence: under random.seed(s) these are the reference's orders.  Returns T rows of T indices."""
    import random
    lst = list(range(T))
    rows = []
    for _ in range(T):
        random.shuffle(lst)
        rows.append(list(lst))
    return rows


class OneList:
    """One stream: the whole step replayed as one Segments (whole_step_calls)."""

    def __init__(self, whole):
        self.whole = whole

    def segments(self):
        return [self.whole]

    def run(self, step_no):
        self.whole.run()


class PCGradSchedule(OneList):
    """The step of a `pcg` model with optim_config["pcgrad_objectives"] = "per_task" (reference model/optimizer.py:10-138,
    fed the list of per-task loss terms): ONE forward, then per objective t
        mask <- 1 in head t's column, 0 elsewhere; labels the heads read <- y * mask   (a zero seed, a zero loss term and
                                                                                         a zero prediction for the others)
        heads + loss, backward chain, table scatter, weight gradients                  (the plan's own lists, replayed)
        predictions and loss term added to the step's totals
        the MLP arena -> bank t; the table rows the scatter marked -> bank t, and cleared  (mml_pcgrad_stash)
    then mml_pcgrad_gram / _weights / _combine over the banks -- the merged gradient lands in the ordinary gradient
    buffers -- and the unchanged optimizer calls.  One stream, one call list (`whole`: one HIP graph).  `order` (the step's
    projection orders) is a plan-owned device buffer run() fills before launching."""

    def __init__(self, plan, store, opt, opt_split, use_graph):
        from . import _lib as L
        from . import bind, ops
        T, B, dev = plan.pcgrad_T, plan.B, plan.device
        if T > L.PCGRAD_MAX_TASKS:
            raise NotImplementedError(f"PCGrad per_task: {T} tasks (at most {L.PCGRAD_MAX_TASKS})")
        if E.has_py(plan.fwd + plan.head_train + plan.bwd + plan.bwd_tail + plan.bwd_side):
            raise NotImplementedError("PCGrad per_task: a plan with Python-issued entries (multi-GPU)")
        self.T = T
        gop = plan.ops[0] if plan.ops else None
        gm = getattr(gop, "grad_marks", None)
        if gm is None and opt.table_update != "dense_exact":
            raise NotImplementedError(f"PCGrad per_task with table_update={opt.table_update!r} needs the scatter's row marks "
                                      "(embedding size 4, 8 or 16, one table per field): use table_update='dense_exact'")
        dd = getattr(gop, "det_deferred", None)
        if dd is not None:
            raise L.MMLError("PCGrad per_task: the deterministic scatter must fold its totals itself (fp32 rows for the banks)")
        reach = E.pcgrad_reach(plan)
        marks_of = store.grad_marks_by_table(gop)
        tabs = [store.pvals[n] for n in store.table_names if store.pvals[n].written]
        # memory: T banks of the MLP arena + T banks of every table's gradient rows (only marked rows are ever touched)
        self.dense_bank = torch.empty((T, store.arena.numel()), dtype=torch.float32, device=dev)
        self.table_banks = {n: torch.empty((T,) + tuple(store.pvals[n].data.shape), dtype=torch.float32, device=dev)
                            for n in store.table_names if store.pvals[n].written}
        self.segs = E.pcgrad_segments(plan, store, reach, self.dense_bank, self.table_banks, marks_of)
        self.gram = torch.zeros((T, T), dtype=torch.float64, device=dev)
        self.w = torch.zeros(2 * T, dtype=torch.float32, device=dev)
        self.fired = torch.zeros((T, T), dtype=torch.int32, device=dev)
        self.order = torch.zeros((T, T), dtype=torch.int32, device=dev)
        self.order_host = [torch.zeros((T, T), dtype=torch.int32).pin_memory() for _ in range(2)]
        self.order_ev = [None, None]
        self.orders = None  # the orders of the latest step (host list)
        # the heads keep reading the label buffer the plan was recorded with; the batch is loaded into a buffer of its own
        self.y_heads = plan.y
        plan.y = plan.zeros(B, T)
        ones, zeros = plan.zeros(B, 1) + 1.0, plan.zeros(B, 1)
        plan.keep += [ones, zeros]
        self.prob_sum, self.loss_sum = plan.zeros(B, T), plan.zeros(1, 1)

        def copies(pairs, accumulate=False):  # one mml_copy2d_batch launch (every src has its dst's shape)
            return E._copy2d_batch_call(plan, pairs, accumulate=[accumulate] * len(pairs))

        table_segs = [[dict(banks=[pv.grad], out=self.table_banks[pv.name][t], marks=marks_of.get(id(pv))) for pv in tabs]
                      for t in range(T)]
        loss2d = plan.loss.view(1, 1)
        self.passes = []
        for t in range(T):
            cols = [(ones, plan.mask[:, t:t + 1])]
            if T > 1:
                prev = (t - 1) % T  # (pass 0: the column the previous step's last pass left set)
                cols.append((zeros, plan.mask[:, prev:prev + 1]))
            calls = [copies(cols),
                     plan.bound(bind.ew_mul(plan.y, plan.mask, self.y_heads), kernel="ew_mul_kernel", bytes=12.0 * B * T)]
            calls += plan.head_train + plan.bwd + plan.bwd_tail + list(getattr(plan, "head_side", [])) + plan.bwd_side
            calls.append(copies([(plan.prob, self.prob_sum), (loss2d, self.loss_sum)], accumulate=t > 0))
            a = ops.make_pcgrad_segs([dict(banks=[store.arena], out=self.dense_bank[t])], 1, need_out=True)
            calls.append(plan.bound(bind.pcgrad_stash(a, 1, False), kernel="pcgrad_stash_kernel",
                                    bytes=8.0 * store.arena.numel()))
            if tabs:
                b = ops.make_pcgrad_segs(table_segs[t], 1, need_out=True)
                calls.append(plan.bound(bind.pcgrad_stash(b, len(tabs), True), kernel="pcgrad_stash_kernel",
                                        bytes=12.0 * B * len(tabs) * tabs[0].data.shape[1]))
            self.passes.append(calls)
        arr = ops.make_pcgrad_segs(self.segs, T, need_out=True)
        n = len(self.segs)
        ws = plan.workspace(L.load().mml_pcgrad_workspace_bytes(arr, n, T), least=256)
        plan.keep += [self.dense_bank, self.table_banks, self.gram, self.w, self.fired, self.order]
        elems = float(sum(int(sg["out"].numel()) if sg.get("marks") is None else
                          min(int(sg["out"].numel()), B * int(sg["out"].shape[1])) for sg in self.segs))
        self.surgery = [
            copies([(self.prob_sum, plan.prob), (self.loss_sum, loss2d)]),
            plan.bound(bind.pcgrad_gram(arr, n, T, self.gram, ws), kernel="pcgrad_gram_kernel", bytes=4.0 * T * elems),
            plan.bound(bind.pcgrad_weights(self.gram, self.order, T, self.w, self.fired), kernel="pcgrad_weights_kernel",
                       bytes=8.0 * T * T),
            plan.bound(bind.pcgrad_combine(arr, n, T, self.w), kernel="pcgrad_combine_kernel",
                       bytes=4.0 * (T + 1) * elems),
        ]
        # the marked dense update clears the scatter's marks itself; the row-wise updates do not read them
        self.unmark = []
        if gm is not None and opt.table_update != "dense_exact":
            z = torch.zeros((gm.numel() // 32, 8), dtype=torch.float32, device=dev)  # (the map is padded to 32 bytes per table)
            plan.keep.append(z)
            self.unmark = [plan.bound(bind.copy2d(z, gm.view(torch.float32).view_as(z), False), kernel="copy2d_kernel",
                                      bytes=2.0 * gm.numel())]
        self.gradients = plan.fwd + [c for p_ in self.passes for c in p_] + self.surgery
        self.calls = (opt_split["pre"] + self.gradients + self.unmark + opt_split["tables"] + opt_split["mlp"])
        OneList.__init__(self, Segments(self.calls, use_graph))

    def run(self, step_no):
        self.upload_orders(step_no)
        self.whole.run()

    def upload_orders(self, step_no):
        """Draw this step's orders on the host and queue their upload in front of the step (two pinned buffers in turn: the
        host may run one step ahead of the device)."""
        k = step_no % 2
        if self.order_ev[k] is not None:
            self.order_ev[k].synchronize()
        self.orders = draw_pcgrad_orders(self.T)
        self.order_host[k].copy_(torch.tensor(self.orders, dtype=torch.int32))
        self.order.copy_(self.order_host[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self.order_ev[k] = ev


def whole_step_calls(p, opt, ar, placement=0, fork_mlp=False, shared_scratch=(), make_fork=None):
    """The whole step as ONE call list (one HIP graph when it holds no Python-issued entry -- every graph seam is ~16 us of
    idle stream, a tenth of a small-batch step) -> (calls, fork_refused).  p: the plan's lists; opt: the optimizer's
    pre / early / mlp / tables lists; ar: [the all-reduce entry] or [].  Unforked:
        pre + fwd + head_train + bwd + bwd_tail + tables + head_side + bwd_side + ar + mlp
    Forked (placement 1, 2 or 3), the side calls head_side + bwd_side run on the fork's branch and the list reads
        1: ... bwd + [fork] + bwd_tail + [join] + tables + ar + mlp        (beside the scatter only)
        2: ... bwd + [fork] + bwd_tail + tables + [join] + ar + mlp        (the default form)
        3: ... bwd + bwd_tail + [fork] + tables + [join] + ar + mlp        (forked behind the scatter)
    fork_mlp without an all-reduce: the MLP optimizer goes behind the weight gradients on their branch (it needs nothing of
    the other one).  The fork is taken iff there are side calls, neither they nor bwd_tail + tables hold a Python-issued
    entry (fork and join must land in ONE graph) and fork_conflicts sees no shared buffer; fork_refused is what it saw (a
    step whose branches share a buffer simply runs unforked).  make_fork(side calls) -> (fork entry, join entry)."""
    head_side = list(getattr(p, "head_side", []))
    mlp_side = bool(fork_mlp) and not ar
    side = head_side + p.bwd_side + (opt["mlp"] if mlp_side else [])
    mid = p.bwd_tail + opt["tables"]
    lead = opt["pre"] + p.fwd + p.head_train + p.bwd
    refused = []
    if placement in (1, 2, 3) and side and not E.has_py(side) and not E.has_py(mid):
        refused = fork_conflicts(side, mid, shared_scratch)
        if not refused:
            fork, join = make_fork(side)
            mid = ([fork] + p.bwd_tail + [join] + opt["tables"]) if placement == 1 else \
                ([fork] + p.bwd_tail + opt["tables"] + [join]) if placement == 2 else \
                (p.bwd_tail + [fork] + opt["tables"] + [join])
            return lead + mid + ar + ([] if mlp_side else opt["mlp"]), refused
    return lead + mid + head_side + p.bwd_side + ar + opt["mlp"], refused


def early_stream_wait(overlap, split_dense, wait_entry):
    """-> (whether the early table pass runs on a stream of its own, what `tail` holds in front of the table update).  The
    pass gets its stream only in a two-stream step whose dense update is split; the touched-row update then waits for it."""
    own = bool(overlap and split_dense)
    return own, ([wait_entry] if own else [])


SEGMENT_NAMES = ("pre", "early", "front", "front_b", "side_a", "sideq", "tail")


def segmented_step(p, opt, ar, wait, split, marks_rows, k, use_graph):
    """The step cut for two streams -> {name: Segments or None} over SEGMENT_NAMES.  split: the dense table update runs as
    an early pass over the untouched rows + a touched-row update; marks_rows: the gather that opens `fwd` lists the batch's
    rows itself (gather + compaction: two entries); k: the early fork's index into bwd (0 = none); wait: [the entry that
    waits for the early pass] when that pass has a stream of its own, else [].
    Without an early pass the counter bump / lazy pre-pass simply lead the front graph; with one, `pre` is everything the
    early pass waits for: the counter, and the row list -- from the index pre-pass, or from the marking gather +
    compaction that open the forward (behind the magnitude reset / weight pass: plan.n_pre entries)."""
    n_lead = ((2 if marks_rows else 0) + getattr(p, "n_pre", 0)) if split else 0
    side_a = [c for c in p.bwd_side if E.call_meta(c).get("ready", 1 << 30) <= k] if k else []
    head_side = list(getattr(p, "head_side", []))
    return dict(
        pre=Segments((opt["pre"] + p.fwd[:n_lead]) if split else [], use_graph),
        early=Segments(opt["early"], use_graph, min_calls=1),
        front=Segments(([] if split else opt["pre"]) + p.fwd[n_lead:] + p.head_train + (p.bwd[:k] if k else p.bwd), use_graph),
        front_b=Segments(p.bwd[k:], use_graph, min_calls=1) if k else None,
        side_a=Segments(side_a, use_graph, min_calls=1) if k else None,
        sideq=Segments(head_side + p.bwd_side[len(side_a):] + ar + opt["mlp"], use_graph),
        # (the touched-row update clears the `seen` bits the early pass is still reading: it waits for that pass)
        tail=Segments(p.bwd_tail + wait + opt["tables"], use_graph))


def _cost(c):
    meta = E.call_meta(c)
    return 4e-6 + meta.get("flops", 0.0) / 5e14 + meta.get("bytes", 0.0) / 4e12


def _early_fork(knobs, p, tables, B):
    """Index into plan.bwd at which the side stream forks early (0 = only at the end of the chain).
    MMLREC_EARLY_WGRAD: unset or 0 = off (the default: measured a loss or level on every workload),
    n > 0 = that index, "auto" = where the side calls that are ready by then take about as long as the rest of the
    chain -- but only when the tail (`tables`: the table optimizer's calls) has no dense table stream of the same length
    to put them beside.
    When no long table stream waits in the tail to hide the weight-gradient GEMMs behind (row-wise table updates, small
    tables), the GEMMs whose operands the backward chain has already produced start beside the REST of the chain instead
    -- worth it where that rest holds HBM-bound launches (PepNet's gate products, the gate / head row kernels) that leave
    the matrix pipe idle.  One more graph seam on each stream."""
    env = knobs.early_wgrad
    ready = [E.call_meta(c).get("ready") for c in p.bwd_side]
    if env == "0" or not p.bwd_side or any(r is None for r in ready) or E.has_py(p.bwd):
        return 0
    if ready != sorted(ready):  # (program order: a later side call is never ready before an earlier one)
        return 0
    if env != "auto":
        return max(0, min(int(env), len(p.bwd) - 1))
    side_t = sum(_cost(c) for c in p.bwd_side)
    table_t = sum(_cost(c) for c in tables)
    if knobs.early_wgrad_debug:
        import sys
        print("early fork: side %.0f us, tables %.0f us, chain %.0f us, ready %s of %d" % (
            side_t * 1e6, table_t * 1e6, sum(_cost(c) for c in p.bwd) * 1e6, ready, len(p.bwd)), file=sys.stderr)
    if B < 16384 or table_t > 0.5 * side_t:
        return 0
    best, best_k = 0.0, 0
    for k in sorted(set(ready)):
        if k <= 0 or k >= len(p.bwd):
            continue
        a = sum(_cost(c) for c, r in zip(p.bwd_side, ready) if r <= k)
        rest = sum(_cost(c) for c in p.bwd[k:])
        if min(a, rest) > best:
            best, best_k = min(a, rest), k
    return best_k if best > 40e-6 else 0


class TwoStreams:
    """The lists of segmented_step replayed: pre, [early on a stream of its own], front, [side_a beside front_b], then tail
    on the main stream beside sideq on the side stream (overlap), or tail and sideq in a row (the split dense update on one
    stream).
    With two streams the step is THREE single-stream graph sequences (front, side, tail) forked and joined with events
    at replay time, not one graph with two branches: hipGraphLaunch of a multi-branch graph walks past the end of the
    exec's parallel-stream vector when one of those streams shares a hardware queue with the launch stream
    (hip::Graph::UpdateStreams, ROCm 7.0 runtime bundled with torch 2.10) -- a sporadic segfault that depends on how many
    streams the process has created.  Single-branch graphs never enter that loop."""

    def __init__(self, device, segs, overlap, early_stream, knobs, single_gpu):
        self.segs = segs  # (TrainStep's: pre, early, front, front_b, side_a, sideq, tail)
        self.overlap = overlap
        self.side = ops_concurrent_stream(device) if overlap else None
        self.tail_stream = None
        if overlap and knobs.cu_tail > 0 and single_gpu:
            from . import ops
            ncu = torch.cuda.get_device_properties(device).multi_processor_count
            self.tail_stream = ops.cu_range_stream(device, 0, knobs.cu_tail)
            self.side = ops.cu_range_stream(device, knobs.cu_tail, ncu)
            self.ev_tail = torch.cuda.Event()
        # (a high-priority stream, or more hardware queues (GPU_MAX_HW_QUEUES=8), for the early pass made a B = 4 096
        # step twice as slow: 0.82 -> 1.6 ms; the default priority it is)
        self.side2 = torch.cuda.Stream(device=device) if early_stream else None
        if early_stream and knobs.cu_early > 0:
            from . import ops
            self.side2 = ops.cu_range_stream(device, 0, knobs.cu_early)
        # fork / join events live as long as the step
        self.ev_fork = torch.cuda.Event() if overlap else None
        self.ev_join = torch.cuda.Event() if overlap else None
        self.ev_pre = torch.cuda.Event() if early_stream else None
        self.ev_early = torch.cuda.Event() if early_stream else None
        self.ev_fork_a = torch.cuda.Event() if segs["front_b"] is not None else None

    def segments(self):
        return [self.segs[n] for n in SEGMENT_NAMES if self.segs[n] is not None]

    def wait_early(self):
        torch.cuda.current_stream().wait_event(self.ev_early)

    def _forked(self, side, tail):
        main = torch.cuda.current_stream()
        self.ev_fork.record(main)
        self.side.wait_event(self.ev_fork)
        with torch.cuda.stream(self.side):
            side()
            self.ev_join.record(self.side)
        if self.tail_stream is not None:
            self.tail_stream.wait_event(self.ev_fork)
            with torch.cuda.stream(self.tail_stream):
                tail()
                self.ev_tail.record(self.tail_stream)
            main.wait_event(self.ev_tail)
        else:
            tail()
        main.wait_event(self.ev_join)

    def run(self, step_no):
        s = self.segs
        s["pre"].run()
        if self.side2 is not None:  # untouched table rows: their own stream, beside everything up to the row update
            main = torch.cuda.current_stream()
            self.ev_pre.record(main)
            self.side2.wait_event(self.ev_pre)
            with torch.cuda.stream(self.side2):
                s["early"].run()
                self.ev_early.record(self.side2)
        else:
            s["early"].run()
        s["front"].run()
        if s["front_b"] is not None:  # early fork: ready weight-gradient GEMMs beside the rest of the backward chain
            main = torch.cuda.current_stream()
            self.ev_fork_a.record(main)
            self.side.wait_event(self.ev_fork_a)
            with torch.cuda.stream(self.side):
                s["side_a"].run()
            s["front_b"].run()
        if not self.overlap:
            s["tail"].run()
            s["sideq"].run()
        else:
            self._forked(s["sideq"].run, s["tail"].run)


class TrainStep:
    """Records the plan of one batch size, asks the optimizer for its lists, builds ONE schedule (PCGradSchedule, OneList
    or TwoStreams) and replays it.  want_overlap / want_split are what the caller asked for (BaseModel.train_step_runner
    caches by them), overlap / split_dense what the step does."""

    def __init__(self, model, B, use_graph=True, allreduce=None, overlap=None, split_dense=True):
        knobs = self.knobs = StepKnobs.from_env()
        self.want_overlap = overlap = resolve_overlap(overlap)
        self.want_split = split_dense
        # PCGrad per-task step (PCGradSchedule): a schedule of its own -- one stream, no split table update, no inner fork
        pcg = getattr(model, "_pcgrad_objectives", lambda: None)() == "per_task"
        par = getattr(model, "_parallel", None)
        if pcg:
            if par is not None or allreduce is not None:
                raise NotImplementedError("the PCGrad per-task step runs on one GPU")
            overlap = False
        self.model = model
        self.store = model._store()
        self.opt = model.optimizer()
        self.par = par
        if allreduce is None and par is not None:
            from .parallel import make_allreduce
            allreduce = make_allreduce(par)
        self.allreduce = allreduce  # callable(flat dense-gradient arena) or None
        self.use_graph = bool(use_graph)
        split = self._record(model, B, pcg, overlap, split_dense, knobs)
        p = self.plan
        # every weight-gradient GEMM of the step in one launch: at small batches (a layer's launch does not fill the chip)
        # and whenever no table stream runs beside them (same-box A/B at B = 65 536: lazy_exact 1.677 -> 1.628 ms, but
        # dense_exact 1.94 -> 1.98: next to the dense table update the per-layer order shares the chip better)
        # Round 5, ONE stream (no table update beside the weight gradients): merged at every batch -- the per-layer
        # launches of a large batch do not all fill the chip either (AE-30's tower layers: 2 tiles x 64 slabs = 128
        # workgroups for 512 slots), and one reduction over 17 slabs replaces three over 25 / 64 / 64.
        self.wgrad_merged = (int(B) <= 8192 or self.opt.table_update != "dense_exact" or not overlap) and \
            knobs.merge_wgrad and passes.merge_wgrad(p)
        if not overlap and knobs.merge_wgrad:
            passes.merge_wgrad16(p)  # (the bf16-storage path's launches: csrc/gemm16.hip)
        opt = self.opt_split = self.opt.calls_split(p, split_dense=split)
        if pcg and self.opt.table_update == "sparse_rows":
            opt["pre"] = opt["pre"] + self.opt.index_pre_calls(p)
        self.split_dense = bool(opt["early"])
        self.opt_calls = opt["pre"] + opt["early"] + opt["mlp"] + opt["tables"]
        # Two streams pay when there is a long table stream to put beside the weight-gradient GEMMs.  The row-wise table
        # updates have none, and at small batches the fork / join (two more graph seams, ~16 us each) costs more than
        # the overlap returns -- same-box A/B, lazy_exact on AE-30: 0.374 forked vs 0.338 ms serial at B = 4 096, level
        # at 16 384, 1.655 vs 1.682 at 65 536 (dense_exact: forked wins at every batch).
        if overlap and self.opt.table_update != "dense_exact" and int(B) <= 8192 and par is None and allreduce is None:
            overlap = False
        self.overlap = bool(overlap)
        ar = [(E.PY, self._allreduce, (), dict(kernel="all_reduce(mlp grads)"))] if allreduce is not None else []
        early_stream, wait = early_stream_wait(self.overlap, self.split_dense,
                                               (E.PY, self._wait_early, (), dict(kernel="wait(early table pass)")))
        k = _early_fork(knobs, p, opt["tables"], int(B)) if self.overlap and not self.split_dense else 0
        self.early_fork = k
        segs = segmented_step(p, opt, ar, wait, self.split_dense,
                              getattr(p.ops[0], "mark_rows", None) is not None, k, self.use_graph)
        # (built, and dumped by tools/plan_dump.py, for every step; replayed by TwoStreams only)
        self.pre, self.early, self.front, self.front_b = segs["pre"], segs["early"], segs["front"], segs["front_b"]
        self.side_a, self.sideq, self.tail = segs["side_a"], segs["sideq"], segs["tail"]
        self.whole = self.pcgrad = self.inner_fork = None
        self.fork_refused = []
        if pcg:
            self.schedule = self.pcgrad = PCGradSchedule(p, self.store, self.opt, opt, self.use_graph)
            self.whole = self.pcgrad.whole
        elif not self.overlap and not self.split_dense:
            from . import ops
            calls, self.fork_refused = whole_step_calls(
                p, opt, ar, knobs.fork_placement(B), knobs.fork_mlp, [w.data_ptr() for w in ops._workspaces.values()],
                self._make_fork)
            self.whole = Segments(calls, self.use_graph)
            self.schedule = OneList(self.whole)
        else:
            self.schedule = TwoStreams(self.store.device, segs, self.overlap, early_stream, knobs, par is None)
        self.calls = 0
        self._nX = self._ny = None  # staging buffers of a prefetched batch
        self._has_next = False

    def _record(self, model, B, pcg, overlap, split_dense, knobs):
        """What to record, and the recording: sets plan, tower_head_fused and grad_marks; returns whether the dense table
        update is split."""
        par = self.par
        rows = None
        if (self.opt.table_update == "lazy_exact" and getattr(self.opt, "auto", False) and par is not None and
                par.mode == "table_wise" and self.opt.steps_done == 0 and self.opt.last is None):
            self.opt.table_update = "dense_exact"  # ('auto' picked lazy_exact before the tables were sharded table-wise)
        # (a PCGrad per-task step lists the rows of a sparse_rows update in an index pre-pass too: its scatter runs once per
        # objective and only accumulates and marks)
        lazy = self.opt.table_update == "lazy_exact" or (pcg and self.opt.table_update == "sparse_rows")
        if lazy and par is not None and par.mode == "table_wise":
            raise NotImplementedError("lazy_exact table updates on the table-wise sharded path (use row_sharded)")
        # Split dense table update (optimizer.Optimizer.can_split_dense): the reference-exact dense optimizer as
        #   early : every row the batch does NOT touch (zero gradient), streamed beside the forward / backward,
        #   tables: the touched rows, with their gradients, after the scatter (mml_opt_step_rows)
        # -- the same arithmetic on every row as one dense launch.  Same-box A/B on AE-30: 0.70-0.76 against 0.77 ms at
        # B = 4 096, 1.95-2.01 against 1.92 ms at B = 65 536 (nothing co-resides with the GEMMs: the early pass only
        # adds its bookkeeping).  Since the single launch learnt to skip the gradient read of the rows the scatter did
        # not mark (grad_marks below: 24 instead of 28 bytes per Adam parameter, no extra launch or stream) the two
        # are level at B = 4 096 too (0.767 / 0.769 ms on one box), so the split form only runs on request
        # (split_dense="force").
        split = (split_dense == "force" and not pcg and (par is None or par.mode == "replicated") and
                 not model._pooled_cols() and  # (the pooled gather marks no rows: the single-launch schedule)
                 self.opt.split_dense_ok([model.embedding_size]))
        if self.opt.table_update in ("sparse_rows", "lazy_exact") or split:
            if par is None:
                rows = self.store.ensure_rows(int(B) * max(model._lookups_per_sample(), 1))
            elif par.mode == "row_sharded":  # one flat table: at most every local row is touched
                rows = self.store.ensure_rows(par.sharding.R)
            elif par.mode == "replicated":
                rows = self.store.ensure_rows(par.world * int(B) * max(len(model._sparse_cols()), 1))
            else:  # this rank serves world*B lookups for each of ITS fields
                sp = model._sparse_cols()
                names = [f"embedding_dict.{sp[f].embedding_name}.weight" for f in par.sharding.mine]
                rows = self.store.ensure_rows(par.world * int(B) * max(len(names), 1), names)
        # lazy_exact lists the batch's rows in a pre-pass (before the gather), so the scatter only accumulates
        # single GPU: the gather marks the rows it reads (no separate pass over X); replicated tables need the rows of
        # the GLOBAL batch, listed by the index pre-pass
        # Single-launch dense update: the scatter marks the rows it adds to, the optimizer reads the gradient of those
        # rows only (mml_opt_tensor.grad_marks): 24 instead of 28 bytes per Adam parameter, no extra launch.
        marked = ((self.opt.table_update == "dense_exact" or pcg) and not split and
                  (par is None or par.mode in ("row_sharded", "replicated")) and
                  knobs.grad_marks)
        # one stream (and no split table update, whose early pass forks anyway): the reductions of the head / gate kernels'
        # partial sums are deferred behind the backward chain and merged into ONE launch (passes.merge_row_reduces)
        one_list = not overlap and not split and knobs.merge_reduces
        with E.deferred_reductions(one_list):
            self.plan = model._record(B, True, False, self.store, sparse_rows=None if (lazy or split) else rows,
                                      lazy=lazy or split, mark_rows=rows if (split and par is None) else None,
                                      grad_marks=marked, **(dict(pcgrad=True) if pcg else {}))
        self.tower_head_fused = False
        if one_list:
            # the top of the network -- last tower layer, heads + BCE, the towers' input gradient -- as one launch where
            # the recorded lists hold that pattern (csrc/tower_head.hip; before the reductions are merged: it brings its own)
            self.tower_head_fused = passes.fuse_tower_head(self.plan)
            passes.merge_row_reduces(self.plan)
        self.grad_marks = getattr(self.plan.ops[0], "grad_marks", None) is not None
        return split

    def _make_fork(self, side_calls):
        self.inner_fork = InnerFork(self.store.device, side_calls)
        return (E.INLINE, self.inner_fork.fork, ()), (E.INLINE, self.inner_fork.join, ())

    def prefetch(self, X=None, y=None, fence=None, fill=None):
        """Hand over the NEXT step's batch while this one is still in flight: it is copied into staging buffers (the
        next run() moves it into plan.X / plan.y itself -- do not copy it there as well) and, on row-sharded tables, its
        index-only routing work (distinct rows, owners, per-owner counts incl. their exchange and the host read of the
        split sizes) starts at once on a side stream.  Collective on the multi-GPU paths: every rank calls it at the
        same point.  Optional: a step whose batch was simply copied into plan.X / plan.y routes it itself.
        fill(X_buf, y_buf): instead of X / y, a callable that writes the staging buffers (it runs on the side stream;
        whatever it reads must be complete and must stay alive until the next run())."""
        p = self.plan
        if self._nX is None:
            self._nX, self._ny = torch.empty_like(p.X), torch.empty_like(p.y)
            self._stage_stream = ops_concurrent_stream(p.device)
            self._ev_staged, self._ev_consumed = torch.cuda.Event(), torch.cuda.Event()
            self._ev_consumed.record(torch.cuda.current_stream())
        op = p.ops[0] if p.ops else None
        side = getattr(op, "route_stream", None) or self._stage_stream
        # X / y must be complete when this is called (resident batches, or `fence` = an event recorded after the work
        # that produces them): the copies are NOT queued behind the step that is in flight on the caller's stream --
        # that is the point -- only behind the previous staged batch having been moved into the plan
        if fence is not None:
            side.wait_event(fence)
        side.wait_event(self._ev_consumed)
        with torch.cuda.stream(side):
            if fill is not None:   # the caller writes the staging buffers itself (e.g. index_select from a resident set)
                fill(self._nX, self._ny)
            else:
                self._nX.copy_(X, non_blocking=True)
                self._ny.copy_(y, non_blocking=True)
            if hasattr(op, "prefetch_route"):
                op.prefetch_route(self._nX)
            self._ev_staged.record(side)
        self._has_next = True

    def load(self, X, y):
        """plan.X / plan.y <- the batch (device tensors of the plan's shapes) in ONE launch on the current stream: two
        tensor copies are two launches in front of every step (6 us each at the head of a 1.8 ms step)."""
        from . import _lib as L
        p = self.plan
        if (X.shape != p.X.shape or y.shape != p.y.shape or X.dtype != torch.float32 or y.dtype != torch.float32 or
                X.stride(1) != 1 or y.stride(1) != 1 or X.device != p.X.device or y.device != p.y.device):
            p.X.copy_(X)
            p.y.copy_(y)
            return
        arr = E.copy2d_descs(((X, p.X), (y, p.y)))
        L.check(L.load().mml_copy2d_batch(arr, 2, torch.cuda.current_stream().cuda_stream), "mml_copy2d_batch")

    def drop_prefetch(self):
        self._has_next = False
        op = self.plan.ops[0] if self.plan.ops else None
        if getattr(op, "staged", None) is not None:
            op.staged = None

    def _allreduce(self):
        self.allreduce(self.store.arena)

    def _wait_early(self):
        self.schedule.wait_early()

    def run(self):
        """plan.X / plan.y must hold the batch. After the call plan.prob / plan.loss hold this step's outputs.
        The first call runs eagerly (HIP graph capture needs warmed-up state and does not execute what it records);
        the second call captures, then every call replays."""
        profiling.push("train_step")
        if self._has_next:  # the batch handed over by prefetch()
            main = torch.cuda.current_stream()
            main.wait_event(self._ev_staged)
            self.load(self._nX, self._ny)
            self._ev_consumed.record(main)
            self._has_next = False
        if self.use_graph and self.calls == 1:
            torch.cuda.synchronize()
            _quiesce_collective_watchdog()
            for seg in self.schedule.segments():
                seg.capture()
            torch.cuda.synchronize()
        self.schedule.run(self.calls)
        self._done()

    def run_gradients(self):
        """PCGrad per-task step only, for tests and diagnostics: everything of run() in front of the optimizer, eagerly.
        The merged gradient is left in the ordinary gradient buffers (table accumulators included, which a step expects
        to find all zero): do not call run() on this model afterwards."""
        if self.pcgrad is None:
            raise RuntimeError("run_gradients: not a PCGrad per-task step")
        self.pcgrad.upload_orders(self.calls)
        E.Plan._run(self.pcgrad.gradients)

    def _done(self):
        profiling.pop()
        self.calls += 1
        self.opt.steps_done += 1
        self.opt.dirty = True
        if self.par is not None:
            self.par.dirty = True
