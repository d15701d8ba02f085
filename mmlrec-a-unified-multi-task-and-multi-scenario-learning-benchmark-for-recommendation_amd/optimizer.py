"""Parameter store and optimizer shared by all plans of one model (K8 front end): gradient buffers, optimizer state and
the optimizer's call lists of a step.

What the lists hold is decided by rules that need no GPU and are written once, here: OptKnobs.from_env reads every
MMLREC_* switch of the optimizer; resolve_table_update picks the table-update mode; dense_table_launches plans the
mml_opt_step_dense calls of the dense table update -- a prediction of what the C side launches, built on the constants
and predicates of _lib.py (tests/test_optimizer_plan_cpu.py).  Optimizer.calls_split turns the plan into entries.
"""
import ctypes as C
import dataclasses
import os
import typing

import torch

from . import _lib as L
from . import engine as E
from . import ops
from . import bind


@dataclasses.dataclass(frozen=True)
class OptKnobs:
    """Every environment switch the optimizer reads (from_env: when an Optimizer is constructed, for the first two, and
    once per calls_split; never at import: tests and lab scripts set the variables between constructions)."""
    # MMLREC_LAZY_MIN_PARAMS: 'auto' takes lazy_exact only above this many table parameters.  Small tables: the literal
    # dense update of a few hundred thousand parameters is one short launch, the row bookkeeping of lazy_exact -- mark +
    # compact, catch-up, row update: four launches -- costs more than it saves; KuaiRec-32's 24 k rows x 16: 90 us of
    # bookkeeping against ~5 us, round 5.
    lazy_min_params: int = 1 << 22
    auto_table_update: str = "lazy_exact"  # MMLREC_AUTO_TABLE_UPDATE=dense_exact: the reference's literal schedule
    # MMLREC_EARLY_BLOCKS: the early half of a split update shares the chip with the forward / backward; its grid can be
    # capped (mml_opt_hyper.max_blocks) so that it leaves them wave slots.  Same-box A/B runs (B = 65 536 and 4 096, caps
    # 512 .. 2048) stayed inside the run-to-run noise, so the default is the full grid (0), at which the stream runs at
    # its stand-alone bandwidth.
    early_blocks: int = 0
    # MMLREC_TAIL_BLOCKS (workgroup cap of the unsplit update, 0 = plain loop) / MMLREC_OPT_U (chunks in flight per thread
    # of the marked form).  Round 3: the single marked launch runs beside the weight-gradient GEMMs of the side stream.
    # Every loop form is its own kernel (csrc/optim.hip: the plain loop at 54 VGPRs / 8 waves per SIMD, two chunks per
    # thread at 100 / 4, four at 172 / 2, eight at 256 / 1).  Alone (same box, ms): two chunks 0.39-0.44, plain 0.43-0.49,
    # four chunks 0.47-0.50, eight 0.85.  In the step (three interleaved repetitions on a quiet box): plain 1.928, two
    # chunks 1.912, four chunks under a 3072-workgroup cap 1.883 -- the two-wave form leaves the GEMMs their registers --
    # but on other boxes the three are level within the +-3 % drift of a run.  Default: two chunks on the full grid, the
    # best stream by itself (0.66-0.74 of 8 TB/s) and level in the step.
    tail_blocks: int = 1 << 20
    opt_u: typing.Optional[int] = None
    # MMLREC_OPT_ONE_LAUNCH=1.  Round 6, built and measured, NOT the default: every table in ONE marked streaming launch
    # instead of the streaming launch of the huge tables + a flat launch of the small ones (AE-30: 26 tables, 31-34 us).
    # Two call lists over ONE model replayed in alternating blocks, both orders (tools/lab/ab_inproc.py --shared,
    # profiles/r06_tail_lab.txt): the single launch is 13 us per step SLOWER (workgroups dealt in proportion to the
    # sizes) or 8 us slower (every tensor the grid a launch of its own would get, small tables first: the form kept).
    one_launch: bool = False
    variant: int = 0           # MMLREC_OPT_VARIANT: bit 1 = two chunks per iteration in the unmarked, unsplit stream
    scatter_old: bool = False  # MMLREC_SCATTER_OLD: the appending atomic scatter, whose touched list is reset here
    # MMLREC_OPT_COLD_ROWS=0: the marked streaming launch gets no warm map (mml_opt_tensor.warm_rows) and updates every
    # row, as it did before the map existed (A/B switch; the results are the same bits either way)
    cold_rows: bool = True
    # MMLREC_OPT_COLD_COMPACT=0: the launch walks a warm map byte by byte, chunk by chunk, as before the wave-compacted loop
    # (mml_opt_hyper.cold_loop = 1; A/B switch, the same bits either way)
    cold_compact: bool = True
    # MMLREC_OPT_RESIDENT: the grid of the wave-compacted loop when every tensor of the launch qualifies for it.  1 = one
    # grid sized for the chip, the spans of all tensors dealt to its waves (mml_opt_hyper.cold_loop = 0); 0 = the
    # workgroups of each tensor, as before that grid (cold_loop = 2); 2 = the chip-sized grid with half the workgroups,
    # one round of them (cold_loop = 3).  A/B switch, the same bits in all three.
    resident: int = 1
    # MMLREC_OPT_STEP_CONSTS=0: the step starts with the plain counter bump and every workgroup of the optimizer launches
    # computes Adam's bias terms itself, as before mml_opt_step_begin (A/B switch, the same bits either way)
    step_consts: bool = True

    @classmethod
    def from_env(cls, env=None):
        env = os.environ if env is None else env
        u = env.get("MMLREC_OPT_U")
        return cls(lazy_min_params=int(env.get("MMLREC_LAZY_MIN_PARAMS", str(1 << 22))),
                   auto_table_update=env.get("MMLREC_AUTO_TABLE_UPDATE", "lazy_exact"),
                   early_blocks=int(env.get("MMLREC_EARLY_BLOCKS", "0")),
                   tail_blocks=int(env.get("MMLREC_TAIL_BLOCKS", str(1 << 20))),
                   opt_u=int(u) if u is not None else None,
                   one_launch=env.get("MMLREC_OPT_ONE_LAUNCH", "0") == "1",
                   variant=int(env.get("MMLREC_OPT_VARIANT", "0")),
                   scatter_old=bool(env.get("MMLREC_SCATTER_OLD")),
                   cold_rows=env.get("MMLREC_OPT_COLD_ROWS", "1") != "0",
                   cold_compact=env.get("MMLREC_OPT_COLD_COMPACT", "1") != "0",
                   resident=int(env.get("MMLREC_OPT_RESIDENT", "1")),
                   step_consts=env.get("MMLREC_OPT_STEP_CONSTS", "1") != "0")


TABLE_UPDATES = ("dense_exact", "sparse_rows", "lazy_exact")
BYTES_PER_PARAM = {"sgd": 12, "adam": 28, "adagrad": 20, "rmsprop": 20}  # p, g, m, v read + p, m, v written


def resolve_table_update(kind, requested, widths, one_table_per_field, table_params, table_reg, knobs):
    """The table-update mode of an Optimizer (its docstring).  requested: 'auto' or a mode; widths: the set of embedding
    widths; one_table_per_field: no table is shared between fields; table_params: parameters of all tables; table_reg:
    the tables' regulariser or None.  'auto' = sparse_rows for SGD / Adagrad; for Adam / RMSprop lazy_exact where it is
    available (one width of 4, 8 or 16, one table per field) and pays (more than knobs.lazy_min_params parameters,
    knobs.auto_table_update not dense_exact), else dense_exact; a regulariser on the tables moves every row every step:
    dense_exact.  A requested lazy_exact is sparse_rows for SGD / Adagrad (nothing to replay: zero gradients do not move
    these optimizers)."""
    mode = requested
    if requested == "auto":
        if kind in ("sgd", "adagrad"):
            mode = "sparse_rows"
        else:
            ok = (len(widths) == 1 and widths <= {4, 8, 16} and one_table_per_field and
                  table_params > knobs.lazy_min_params and knobs.auto_table_update == "lazy_exact")
            mode = "lazy_exact" if ok else "dense_exact"
        if table_reg:
            mode = "dense_exact"
    if mode == "lazy_exact" and kind in ("sgd", "adagrad"):
        mode = "sparse_rows"
    if mode not in TABLE_UPDATES:
        raise ValueError("table_update must be auto, dense_exact, sparse_rows or lazy_exact")
    return mode


def opt_dense_symbol(numel, ntensors, form=0, opt_u=None):
    """Kernel symbol of a dense optimizer launch (csrc/opt_plan.hpp: mml_opt_step_dense's choice).  form: the loop form
    of the streaming kernel -- 0 plain, 1 two chunks per iteration (MMLREC_OPT_VARIANT bit 1), 2 untouched rows of the
    split update under a capped grid, 3 marked gradients under a capped grid, 4 marked gradients plus the deferred totals
    of the deterministic scatter (any grid).  opt_u: OptKnobs.opt_u; a value without an instantiation runs two chunks."""
    if not L.opt_dense_streams(numel, ntensors, form in (3, 4)):
        return "opt_flat_kernel"
    u = {0: 1, 1: 1, 2: 4, 3: opt_u if opt_u in (4, 8) else 2, 4: 4 if opt_u == 4 else 2}[form]
    return "opt_dense_kernel<true, %d, %d>" % (form, u)


class DenseLaunch(typing.NamedTuple):
    """One mml_opt_step_dense call of the dense table update: the written tables' indices in launch order, whether the
    launch reads gradient marks, the loop form (opt_dense_symbol), the traffic in bytes and the kernel's symbol."""
    tables: tuple
    marked: bool
    form: int
    bytes: float
    kernel: str


def dense_table_launches(kind, numels, rows, marks, split_dense, cap, det_deferred, knobs, det_exact=True):
    """The launches of the dense table update; one C call = one launch (the size rule mml_opt_step_dense applies inside a
    call, mirrored in _lib.py), so that a call's label is the kernel symbol a profiler reports.
    numels / rows / marks: per written table, in store order, its parameters, its rows and whether the scatter marked its
    gradient's rows; cap: the workgroup cap of the launches' hyper (0 = none); det_deferred: the deterministic scatter
    left its totals to this update (GatherOp.det_deferred), det_exact: the written tables are exactly that gather's.
      * big = the tables of at least 2^22 parameters -- none if they are more than 4 or hold fewer than 2^24 together;
        small = the rest.  The launches are the non-empty ones of (big, small), in that order: the huge tables stream,
        every other table shares one balanced flat launch.
      * one_launch needs all of: big and small both non-empty, cap > 0, at most MAX_OPT_TENSORS tables, not split, every
        table marked, knobs.one_launch.
      * Deferred totals force one_launch -- the flat kernel reads neither marks nor totals -- after the check
        (_lib.opt_takes_det_totals, else MMLError) that the update is not split, covers exactly the gather's tables
        and every table is marked.
      * Under one_launch there is a single launch, small tables first (their workgroups start with the launch), then
        the big ones; it counts as the big launch.
      * marked: only the big launch, and only when all its tables are marked.
      * form: 4 with deferred totals, else 3 if cap > 0 and marked, else 2 if cap > 0 and split, else 1 if
        knobs.variant & 2 and neither marked nor split, else 0.
      * bytes = per-parameter bytes (12 / 28 / 20 / 20 for sgd / adam / adagrad / rmsprop, minus 4 when split: that form
        never reads g) x numel; a marked launch reads g for the marked rows only (~1 %) and the mark bytes instead:
        + sum(rows - 4 numel).
      * kernel = opt_dense_symbol(numel, tables, form, knobs.opt_u)."""
    n = len(numels)
    big = [i for i in range(n) if numels[i] >= L.OPT_HUGE_MIN_PARAMS]
    if len(big) > L.OPT_STREAM_MAX_TENSORS or sum(numels[i] for i in big) < L.OPT_STREAM_MIN_PARAMS:
        big = []
    small = [i for i in range(n) if i not in big]
    one_launch = bool(big and small and cap > 0 and n <= L.MAX_OPT_TENSORS and not split_dense and all(marks) and
                      knobs.one_launch)
    if det_deferred:
        if not (det_exact and L.opt_takes_det_totals(numels, all(marks), split_dense)):
            raise L.MMLError("the deterministic scatter deferred its totals to a marked dense update of exactly its "
                             "tables")
        one_launch = True
    if one_launch:
        big, small = small + big, []
    per = BYTES_PER_PARAM[kind] - (4 if split_dense else 0)
    out = []
    for grp in (big, small):
        if not grp:
            continue
        marked = grp is big and all(marks[i] for i in grp)
        numel = sum(numels[i] for i in grp)
        nbytes = float(per) * numel
        form = (4 if det_deferred else 3 if (cap > 0 and marked) else 2 if (cap > 0 and split_dense) else
                1 if (knobs.variant & 2 and not marked and not split_dense) else 0)
        if marked:
            nbytes += sum(rows[i] - 4.0 * numels[i] for i in grp)
        out.append(DenseLaunch(tuple(grp), marked, form, nbytes, opt_dense_symbol(numel, len(grp), form, knobs.opt_u)))
    return out


WARM_KINDS = ("adam", "rmsprop", "adagrad")


def launch_trusts_warm_map(kind, marked, table_reg, knobs, sharded=False):
    """May a launch of dense_table_launches pass over the rows whose byte in the table's warm map (Optimizer.warm) is 0?
    Only the marked streaming launch reads the map (mml_opt_tensor.warm_rows goes with grad_marks); a row with zero
    moments and a zero gradient stays where it is under Adam / RMSprop / Adagrad and no regulariser (SGD has no moments
    to be zero, and a regulariser moves every row every step); knobs.cold_rows switches the map off, and the sharded
    updates of parallel.py (sharded: the gather is not an engine.GatherOp) do without it.  A launch that may
    not trust the map takes None and, since it writes moments the map does not know of, marks every row of its tables
    warm (Optimizer.all_rows_warm) -- as does every other writer of a table's moments."""
    return bool(marked and kind in WARM_KINDS and not table_reg and knobs.cold_rows and not sharded)


def cold_loop_of(knobs):
    """mml_opt_hyper.cold_loop of the dense table launches: 0 = the wave-compacted loop over a warm map on one grid sized
    for the chip, 1 = the loop before it (knobs.cold_compact off), 2 = the compacted loop on each tensor's own
    workgroups (knobs.resident = 0), 3 = as 0 with half the workgroups (knobs.resident = 2).  A launch without a warm
    map does not look at the field."""
    if not knobs.cold_compact:
        return 1
    return {0: 2, 2: 3}.get(knobs.resident, 0)


def step_pre_entry(lib, step_dev_ptr, consts_ptr, hyper):
    """The entry a step's call list starts with.  With a constants buffer (consts_ptr): mml_opt_step_begin, ONE launch
    that bumps the device step counter and leaves the step's constants (Adam's bias terms) where the optimizer launches
    under `hyper`'s kind / lr / betas read them; without one (None): the plain counter bump, and every workgroup
    computes them.  One entry either way."""
    if consts_ptr is None:
        return (lib.mml_counter_update, (step_dev_ptr, 1, 0))
    return (lib.mml_opt_step_begin, (step_dev_ptr, 1, C.byref(hyper), consts_ptr))


class TableRows:
    """Bookkeeping for the sparse-row table update: per-table `seen` bitmaps + the touched-row list."""

    def __init__(self, vocab, device, cap):
        self.rowbase = [0]
        for v in vocab:
            self.rowbase.append(self.rowbase[-1] + int(v))
        self.seen = [torch.zeros((int(v) + 31) // 32, dtype=torch.int32, device=device) for v in vocab]
        # one byte per row, all-zero between launches: rows are marked with plain stores, a compaction pass turns the
        # marks into the bitmaps + the list (include/mmlrec.h: row_marks)
        self.marks = torch.zeros(ops.marks_bytes(vocab), dtype=torch.uint8, device=device)
        self.touched = torch.zeros(max(int(cap), 1), dtype=torch.int32, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)


class ParamStore:
    """Gradient buffers and optimizer state for one model on one device.

    Dense (MLP) parameter gradients live in ONE flat arena (a single buffer to all-reduce under data parallelism);
    every table gets a dense [V,E] accumulator that is kept all-zero between steps (the optimizer kernels re-zero
    what they consume), so the scatter can add into it without a per-step 400 MB memset."""

    def __init__(self, model, device):
        self.device = device
        self.model = model
        tables, dense = [], []
        for name, p in model.named_parameters():
            (tables if name.startswith("embedding_dict.") else dense).append((name, p))
        self.sig = tuple(p.data_ptr() for _, p in tables + dense)
        total = sum(p.numel() for _, p in dense)
        self.arena = torch.zeros(max(total, 1), dtype=torch.float32, device=device)
        self.pvals = {}
        off = 0
        for name, p in dense:
            g = self.arena[off:off + p.numel()].view(p.shape)
            off += p.numel()
            self.pvals[name] = E.PVal(p.data, g, name)
            self.pvals[name].stable = True
        self.table_names = [n for n, _ in tables]
        for name, p in tables:
            self.pvals[name] = E.PVal(p.data, None, name, is_table=True)
        par = getattr(model, "_parallel", None)
        if par is not None and par.mode == "row_sharded":
            # the trained rows of this rank live in ONE flat buffer (parallel.RowSharding); the full per-field tables
            # stay registered (state_dict / predict contract) but are never written by a step
            self.pvals["embedding_shard"] = E.PVal(par.shard, None, "embedding_shard", is_table=True)
            self.table_names = ["embedding_shard"]
        self.table_grads_ready = False
        self.opt = None
        self.rows = None
        self.rows_names = None
        self._grad_marks_key = self._det_key = None  # the tables grad_marks / _det were made for
        self.extra = {}  # derived / frozen tensors registered by models (STAR)

    def ensure_table_grads(self):
        if not self.table_grads_ready:
            for n in self.table_names:
                pv = self.pvals[n]
                pv.grad = torch.zeros_like(pv.data)
                pv.needs_grad = True
            self.table_grads_ready = True

    def ensure_rows(self, cap, names=None):
        """Touched-row bookkeeping over the tables this rank updates (all of them unless `names` is given)."""
        names = list(self.table_names if names is None else names)
        if self.rows is None or self.rows.touched.numel() < cap or self.rows_names != names:
            self.rows = TableRows([self.pvals[n].data.shape[0] for n in names], self.device, cap)
            self.rows_names = names
        return self.rows

    def ensure_grad_marks(self, tables):
        """Byte map over the rows of `tables` (a gather's field order; ops.marks_bytes layout) for the marked-gradient
        dense update.  Returns (map, byte offset of every table)."""
        vocab = [int(t.data.shape[0]) for t in tables]
        key = tuple(t.data.data_ptr() for t in tables)
        if self._grad_marks_key != key:
            self.grad_marks = torch.zeros(ops.marks_bytes(vocab), dtype=torch.uint8, device=self.device)
            self._grad_marks_key = key
        base, off = [], 0
        for v in vocab:
            base.append(off)
            off += (v + 31) // 32 * 32
        return self.grad_marks, base

    def grad_marks_by_table(self, gop):
        """{id(table): its rows' slice of the mark map} for the tables of a gather whose scatter marks rows; {} for one
        that does not (or for no gather at all)."""
        gm = getattr(gop, "grad_marks", None)
        if gm is None:
            return {}
        _, base = self.ensure_grad_marks(gop.tables)
        return {id(t): gm[base[f]:base[f] + t.data.shape[0]] for f, t in enumerate(gop.tables)}

    def ensure_det(self, tables):
        """Buffers of the deterministic scatter for `tables` (a gather's field order): int64 [V, E] totals per table (kept
        all zero between steps by the scatter's second launch, or by the table optimizer that takes the totals over), a
        mark map of its own and a magnitude slot."""
        key = tuple(t.data.data_ptr() for t in tables)
        if self._det_key != key:
            uniq = {}
            for t in tables:
                uniq.setdefault(t.data.data_ptr(), torch.zeros(t.data.shape, dtype=torch.int64, device=self.device))
            self._det = dict(acc64=[uniq[t.data.data_ptr()] for t in tables],
                             marks=torch.zeros(ops.marks_bytes([int(t.data.shape[0]) for t in tables]), dtype=torch.uint8,
                                               device=self.device),
                             slot=ops.amax_slots(1, self.device)[0])
            self._det_key = key
        return self._det

    def stale(self):
        return self.sig != tuple(p.data_ptr() for _, p in self.model.named_parameters())

    def reset_written(self):
        for pv in self.pvals.values():
            pv.written = 0
        for pv in self.extra.values():
            pv.written = 0


class _OptState(dict):
    """name -> (state1, state2), zero-initialised on first use (a row-sharded run never touches the full tables).

    warm: table name -> uint8 [rows], 0 = the row's moments are still the zeros they were created as.  A table's map is
    born all-zero with its zero moments, here and nowhere else; moments that come from outside (state[name] = ...: a
    loaded checkpoint, a test that plants a state) have no map, and none is made for them later."""

    def __init__(self, store, kind):
        super().__init__()
        self.store, self.kind = store, kind
        self.warm = {}

    def __missing__(self, name):
        pv = self.store.pvals[name]
        s1 = torch.zeros_like(pv.data) if self.kind != "sgd" else None
        s2 = torch.zeros_like(pv.data) if self.kind == "adam" else None
        dict.__setitem__(self, name, (s1, s2))
        if pv.is_table and s1 is not None:
            self.warm[name] = torch.zeros(pv.data.shape[0], dtype=torch.uint8, device=pv.data.device)
        return (s1, s2)

    def __setitem__(self, name, value):
        self.warm.pop(name, None)
        dict.__setitem__(self, name, value)

    def __delitem__(self, name):
        self.warm.pop(name, None)
        dict.__delitem__(self, name)


class Optimizer:
    """K8 front end: dense update for MLP parameters; for the tables one of
      dense_exact : every row every step, like the reference's torch.optim over dense gradients;
      sparse_rows : rows of the batch only -- exactly the dense result for SGD / Adagrad, "lazy Adam" otherwise;
      lazy_exact  : rows of the batch only, but the zero-gradient steps a row skipped are replayed before it is next
                    read (mml_opt_catchup_rows) and for all rows before evaluation (flush): the dense Adam / RMSprop
                    trajectory at sparse cost (SURVEY.md A14 "hard part" solved without changing results).
    'auto' = sparse_rows for SGD / Adagrad (exactly the dense result); for Adam / RMSprop lazy_exact where it is
    available -- embedding width 4, 8 or 16, one table per field, no regulariser on the tables (round 4: the same
    dense trajectory, tests at 2e-6, at 51 M instead of 37 M samples/s on AE-30 incl. the flush of a 500-step epoch) --
    else dense_exact.  MMLREC_AUTO_TABLE_UPDATE=dense_exact keeps the reference's literal schedule under 'auto'
    (resolve_table_update)."""

    def __init__(self, store, kind, lr, table_update="auto"):
        self.store, self.kind, self.lr = store, kind, float(lr)
        if kind not in L.OPT_KINDS:
            raise NotImplementedError(kind)  # model/basemodel.py:581
        self.auto = table_update == "auto"
        tabs = [p for n, p in store.model.named_parameters() if n.startswith("embedding_dict.")]
        cols = store.model._sparse_cols() if hasattr(store.model, "_sparse_cols") else []
        self.table_update = resolve_table_update(
            kind, table_update, widths={int(p.shape[1]) for p in tabs},
            one_table_per_field=len({f.embedding_name for f in cols}) == len(cols),
            table_params=sum(p.numel() for p in tabs), table_reg=self.table_reg() if self.auto else None,
            knobs=OptKnobs.from_env())
        self.last = None   # lazy_exact: per-table int32 [V] "row is current as of step"
        self.dirty = False
        dev = store.device
        self.step_dev, self.step_consts = ops.step_counter(dev)  # (the counter and the step's constants: one allocation)
        self.state = _OptState(store, kind)  # moments are allocated when a tensor is first updated
        self.warm = self.state.warm          # table name -> byte per row: may the row's moments be non-zero?
        self.steps_done = 0

    def __del__(self):
        # the library's (counter -> constants) entry goes with the buffers it names
        try:
            ops.opt_step_unbind(self.step_dev)
        except Exception:  # (interpreter shutdown: nothing left to tidy)
            pass

    def warm_map(self, name):
        """The warm map of table `name` for a launch that honours it (launch_trusts_warm_map), or None when the table's
        moments did not start as zeros of this optimizer's making."""
        self.state[name]
        return self.warm.get(name)

    def all_rows_warm(self, names):
        """Every writer of a table's moments that is not a warm-aware launch calls this when its call list is built (the
        map only ever goes from 0 to 1, so doing it early is safe): from here on no row of these tables is passed over."""
        for n in names:
            self.state[n]
            if n in self.warm:
                self.warm[n].fill_(1)

    def calls(self, plan):
        """Optimizer call list for one step (appended after a plan's backward)."""
        c = self.calls_split(plan)
        return c["pre"] + c["early"] + c["mlp"] + c["tables"]

    def split_dense_ok(self, widths):
        """The optimizer's half of the split predicate: the update is dense_exact, the same function of (p, g, state) in
        both kernels (no regulariser on the tables) and the row kernels serve the embedding widths (mml_index_unique:
        E <= 16, a multiple of 4)."""
        return (self.table_update == "dense_exact" and not self.table_reg() and
                all(w <= 16 and w % 4 == 0 for w in widths))

    def can_split_dense(self, plan):
        """The dense table update may run as (untouched rows early, next to the forward) + (touched rows after the
        scatter): split_dense_ok, and the batch's row set is known before the forward (indices on this rank)."""
        gop = plan.ops[0] if plan.ops else None
        if not isinstance(gop, E.GatherOp) or isinstance(gop, E.PooledGatherOp):  # (the pooled gather marks no rows)
            return False
        return self.split_dense_ok([t.data.shape[1] for t in gop.tables])

    def calls_split(self, plan, split_dense=False):
        """{'pre': step-counter bump (+ the index pre-pass), 'early': the untouched-rows half of a split dense table
        update (may run beside the forward / backward), 'mlp': dense MLP update, 'tables': table update (+ touched-list
        reset)} so a trainer can put them on different streams."""
        knobs = OptKnobs.from_env()
        hyper = ops.make_hyper(self.kind, self.lr, step=0, step_dev=self.step_dev, zero_grad=False)
        plan.keep.append(hyper)
        pre = [step_pre_entry(L.load(), self.step_dev.data_ptr(),
                              self.step_consts.data_ptr() if knobs.step_consts else None, hyper)]
        if self.table_update == "lazy_exact":
            pre += self._lazy_pre_calls(plan)
        split_dense = bool(split_dense) and self.can_split_dense(plan)
        if split_dense and getattr(plan.ops[0], "mark_rows", None) is None:  # (else the gather itself lists the rows)
            pre += self.index_pre_calls(plan)
        reg = self._reg_map()
        treg = self.table_reg(reg)
        names = [n for n in self.store.table_names if self.store.pvals[n].written]
        if treg and self.table_update != "dense_exact":
            raise NotImplementedError("l2_reg_embedding / l1 on the tables makes every row's gradient non-zero: use "
                                      "table_update='dense_exact' (the reference's own dense optimizer)")
        mlp = self._mlp_calls(plan, reg, hyper)
        early, tables = [], []
        if names and self.table_update == "dense_exact":
            (early if split_dense else tables).extend(self._dense_table_calls(plan, names, treg, split_dense, knobs))
        if names and (self.table_update != "dense_exact" or split_dense):
            tables += self._row_update_calls(plan, names, hyper, knobs)
        return {"pre": pre, "early": early, "mlp": mlp, "tables": tables}

    def _mlp_calls(self, plan, reg, hyper):
        """The dense update of the MLP parameters: one mml_opt_step_dense entry (none without parameters)."""
        # (a regularised parameter is updated even when no gradient reaches it -- the reference's dead PLE tensors,
        # its arena slice stays zero, the update sees the regulariser's gradient alone)
        dense = [(pv, n) for n, pv in self.store.pvals.items()
                 if not pv.is_table and pv.grad is not None and (pv.written or pv.data.data_ptr() in reg)]
        if not dense:
            return []
        arr = ops.make_opt_tensors([(pv.data, pv.grad) + self.state[n] + (reg.get(pv.data.data_ptr()),)
                                    for pv, n in dense])
        plan.keep.append(arr)
        numel = sum(pv.data.numel() for pv, _ in dense)
        return [(L.load().mml_opt_step_dense, (arr, len(dense), C.byref(hyper)),
                 dict(kernel=opt_dense_symbol(numel, len(dense)), bytes=float(BYTES_PER_PARAM[self.kind]) * numel))]

    def _dense_table_calls(self, plan, names, treg, split_dense, knobs):
        """dense_exact: one mml_opt_step_dense entry per launch of dense_table_launches over the written tables."""
        st = self.store
        tabs = [st.pvals[n] for n in names]
        cap = knobs.early_blocks if split_dense else knobs.tail_blocks
        hz = ops.make_hyper(self.kind, self.lr, step=0, step_dev=self.step_dev, zero_grad=not split_dense,
                            max_blocks=cap, cold_loop=cold_loop_of(knobs))
        plan.keep.append(hz)
        seen_of = dict(zip(st.rows_names, st.rows.seen)) if split_dense else {}
        # marked gradients (the scatter of this plan marked every row it added to): the streaming launch does not
        # read the gradient of unmarked rows -- 24 instead of 28 bytes per Adam parameter
        gop = plan.ops[0] if plan.ops else None
        marks_of = {} if split_dense else st.grad_marks_by_table(gop)
        # Deterministic scatter with deferred totals (GatherOp.det_deferred): the scatter's second launch is folded
        # into the ONE marked streaming launch, which adds the marked rows' 64-bit totals to the gradient it reads
        # (mml_opt_tensor.acc64)
        dd = getattr(gop, "det_deferred", None)
        launches = dense_table_launches(
            self.kind, [t.data.numel() for t in tabs], [t.data.shape[0] for t in tabs],
            [id(t) in marks_of for t in tabs], split_dense, cap, dd is not None, knobs,
            det_exact=dd is None or {id(t) for t in tabs} == {id(t) for t in gop.tables})
        acc_of = {id(t): a for t, a in zip(gop.tables, gop.deterministic["acc64"])} if dd else {}
        calls = []
        for ln in launches:
            # rows whose moments are still zero and whose gradient is unmarked are not even read (mml_opt_tensor.warm_rows)
            trust = launch_trusts_warm_map(self.kind, ln.marked, treg, knobs, sharded=not isinstance(gop, E.GatherOp))
            if not trust:
                self.all_rows_warm([names[i] for i in ln.tables])
            arr = ops.make_opt_tensors([(tabs[i].data, tabs[i].grad) + self.state[names[i]] +
                                        (treg, seen_of.get(names[i]), marks_of[id(tabs[i])] if ln.marked else None,
                                         (acc_of[id(tabs[i])], dd["slot"], dd["shift"]) if dd else None,
                                         self.warm_map(names[i]) if trust else None)
                                        for i in ln.tables])
            plan.keep.append(arr)
            m = dict(kernel=ln.kernel, bytes=ln.bytes)
            if dd:  # (+ 32 bytes of totals read and zeroed per 16-byte chunk of a marked row; the buffers the
                # descriptors hide from trainer.fork_conflicts)
                m.update(det_acc64=True, ptrs=[dd["slot"].data_ptr()] + [a.data_ptr() for a in acc_of.values()])
            calls.append((L.load().mml_opt_step_dense, (arr, len(ln.tables), C.byref(hz)), m))
        return calls

    def _row_update_calls(self, plan, names, hyper, knobs):
        """The row update over the touched list (sparse_rows, lazy_exact, the touched half of a split dense update) and,
        for the appending scatter only, the list's reset."""
        rows = self.store.rows
        tabs = [self.store.pvals[n] for n in names]
        self.all_rows_warm(names)  # (the row kernels write moments and know no warm map)
        calls = [plan.bound(bind.opt_step_rows([t.data for t in tabs], [t.grad for t in tabs], *self._moments(names),
                                               bind.rows_args(rows), hyper,
                                               last=[self.last[n] for n in names] if self.table_update == "lazy_exact"
                                               else None), kernel="opt_rows_kernel")]
        # the list is REBUILT every step by the compaction that follows the marking kernels (E in 4, 8, 16: it
        # resets the counter itself); only the appending atomic path needs the reset here
        if tabs[0].data.shape[1] not in (4, 8, 16) or knobs.scatter_old:
            calls.append(plan.bound(bind.counter_update(rows.count, 0, True)))
        return calls

    def _moments(self, names):
        """(state1, state2) of the tables `names` as the row kernels take them: a list per moment the optimizer kind keeps,
        None for the others."""
        return ([self.state[n][0] for n in names] if self.kind != "sgd" else None,
                [self.state[n][1] for n in names] if self.kind == "adam" else None)

    def _index_unique_entry(self, plan, gop):
        """The batch's distinct rows -> `seen` bitmaps + touched list, over every table of the store."""
        st = self.store
        tabs = [st.pvals[n] for n in st.table_names]
        X, nrows = gop.index_view(plan)
        return plan.bound(bind.index_unique([t.data.shape[0] for t in tabs], gop.cols, tabs[0].data.shape[1], X,
                                            bind.rows_args(st.rows), plan.status, B=nrows),
                          kernel="mark_rows_kernel+rows_compact_kernel", bytes=float(nrows) * len(tabs) * 5)

    def index_pre_calls(self, plan):
        """Index pre-pass of the split dense update (and of a PCGrad per-task step over sparse_rows): the batch's distinct
        rows -> `seen` bitmaps + touched list."""
        st, gop = self.store, plan.ops[0]
        if st.rows is None or list(st.rows_names) != list(st.table_names):
            raise L.MMLError("split dense update needs ParamStore.ensure_rows over every table")
        return gop.pre_index_calls(plan) + [self._index_unique_entry(plan, gop)]

    # ---- regulariser (model/basemodel.py:524-540) ---------------------------------------------------------
    def _reg_map(self):
        """data_ptr -> (l1, l2) summed over the groups the model registered with add_regularization_weight."""
        out = {}
        for weight_list, l1, l2 in getattr(self.store.model, "regularization_weight", []):
            if not (l1 > 0 or l2 > 0):
                continue
            for w in weight_list:
                p = w[1] if isinstance(w, tuple) else w
                a, b = out.get(p.data_ptr(), (0.0, 0.0))
                out[p.data_ptr()] = (a + float(l1), b + float(l2))
        return out

    def table_reg(self, reg=None):
        """(l1, l2) of the embedding tables (one setting for all of them: l2_reg_embedding), or None.  reg: a _reg_map
        already at hand."""
        reg = self._reg_map() if reg is None else reg
        vals = {reg[p.data_ptr()] for n, p in self.store.model.named_parameters()
                if n.startswith("embedding_dict.") and p.data_ptr() in reg}
        if not vals:
            return None
        if len(vals) > 1:
            raise NotImplementedError("different regularisers on different embedding tables")
        return vals.pop()

    # ---- lazy_exact ----------------------------------------------------------------------------------
    def _lazy_pre_calls(self, plan):
        """Before the gather: unique rows of the batch (LDS dedup on the indices) -> replay their skipped steps."""
        lib, st = L.load(), self.store
        gop = plan.ops[0]
        names = st.table_names
        rows = st.rows
        if self.last is None:
            self.last = {n: torch.zeros(st.pvals[n].data.shape[0], dtype=torch.int32, device=st.device) for n in names}
        tabs = [st.pvals[n].data for n in names]
        ra = bind.rows_args(rows)
        self.all_rows_warm(names)  # (the catch-up writes moments)
        hyper = ops.make_hyper(self.kind, self.lr, step=0, step_dev=self.step_dev)
        catchup = plan.bound(bind.opt_catchup_rows(tabs, *self._moments(names), [self.last[n] for n in names], ra, hyper),
                             kernel="opt_catchup_kernel")
        if getattr(gop, "owns_lazy", False):
            # row-sharded tables: the keys to bring up to date only exist on the owner after the index exchange, so
            # the gather op launches (unique -> catch-up) itself, on the flat shard (F == 1)
            if len(tabs) != 1:
                raise L.MMLError("row-sharded lazy_exact expects the single flat shard")
            vocab, Em = (L.i64 * 1)(tabs[0].shape[0]), tabs[0].shape[1]

            def launch(keys_ptr, n, stream):
                if n:
                    L.check(lib.mml_index_unique_idx32(vocab, 1, Em, keys_ptr, 1, n, *ra, plan.status.data_ptr(),
                                                       stream), "mml_index_unique_idx32")
                    L.check(catchup[0](*catchup[1], stream), "mml_opt_catchup_rows")
            gop.lazy_launch = launch
            return []
        if not isinstance(gop, E.GatherOp):
            raise L.MMLError("lazy_exact table updates are not available on the table-wise sharded path")
        if isinstance(gop, E.PooledGatherOp):
            return gop.pre_index_calls(plan) + gop.unique_calls(plan, rows) + [catchup]
        return gop.pre_index_calls(plan) + [self._index_unique_entry(plan, gop), catchup]

    def flush(self):
        """Bring EVERY table row to the current step (needed before anything outside the fused step reads a table)."""
        if self.table_update != "lazy_exact" or not self.dirty or self.last is None:
            return
        hyper = ops.make_hyper(self.kind, self.lr, step=0, step_dev=self.step_dev)
        self.all_rows_warm(self.store.table_names)
        for n in self.store.table_names:
            s1, s2 = self.state[n]
            ops.opt_catchup_dense(self.store.pvals[n].data, s1, s2 if self.kind == "adam" else None, self.last[n], hyper)
        self.dirty = False
