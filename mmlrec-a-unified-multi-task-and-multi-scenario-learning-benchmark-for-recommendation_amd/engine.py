"""Static step plans: a model's forward is recorded ONCE per batch size as a short list of C-ABI calls on
pre-allocated device buffers, its backward is derived from that record, and a training step is
`fwd calls + fused head/BCE call + bwd calls + optimizer calls` -- about 25 kernel launches for MMoE instead of
the ~1 000 ATen ops the reference issues per step.  The call list is replayable inside a HIP graph
(torch.cuda.CUDAGraph is used purely as the capture/replay plumbing).

Gradient convention: `Val.grad` holds dL/d(pre-activation) once every consumer has contributed.  A consumer that is
the ONLY consumer of a value folds the activation derivative into its own kernel epilogue (dgrad / gate / head
kernels do this); otherwise consumers add raw contributions and one `mml_act_bwd` pass finalises the sum.
"""
import contextlib
import ctypes as C
import dataclasses
import os
import typing

import torch

from . import _lib as L
from . import profiling
from . import ops
from . import bind

ACT = {"none": L.ACT_NONE, None: L.ACT_NONE, "linear": L.ACT_NONE, "relu": L.ACT_RELU, "sigmoid": L.ACT_SIGMOID,
       "sigmoid2": L.ACT_SIGMOID2}
# PReLU is not an MML_ACT_* code (no GEMM epilogue applies it): the layer's Linear / BatchNorm runs with ACT_NONE and a
# PReluBatchOp follows.  The marker never reaches a kernel descriptor.
ACT_PRELU = 100
ACT["prelu"] = ACT_PRELU


class PVal:
    """A parameter tensor (or a tensor derived from parameters) with an optional gradient buffer."""

    def __init__(self, data, grad=None, name="", needs_grad=True, is_table=False):
        self.data, self.grad, self.name = data, grad, name
        self.needs_grad = needs_grad and grad is not None
        self.is_table = is_table
        self.written = 0  # build-time counter: first writer overwrites, later writers accumulate
        # True: a trained parameter (optimizer.ParamStore) that changes only in the optimizer -- its magnitude is measured ONCE at
        # the start of a step.  False: a tensor some op of the step produces (STAR's effective weights, APG's generated
        # ones): measured where it is used.
        self.stable = False


class Val:
    """A [B, n] activation living in a (possibly column-sliced) device buffer."""

    def __init__(self, buf, act=L.ACT_NONE, needs_grad=True, name=""):
        self.buf, self.act, self.needs_grad, self.name = buf, act, needs_grad, name
        self.grad = None
        self.consumers = []  # ops that would write a gradient into this value
        self.written = 0
        self.deriv_applied = False
        self.mask = None  # int32 [B, ceil(n/32)] relu sign bits (training plans, written by the producing GEMM)
        # > 0: the value owns its rows up to column kpad (a multiple of 16) and the columns [n, kpad) are zero and
        # never written -- a GEMM may then read it as a [B, kpad] operand (LinearGroupOp: reduction lengths that
        # are not a multiple of the 16-wide k-step, e.g. 30 x 8 embedding columns + 63 dense columns = 303)
        self.kpad = 0
        # > 0: only the first grad_cols columns of the gradient have a reader (dnn_input: the table scatter reads the
        # embedding columns, nobody the dense features' -- model/basemodel.py:461-487 concatenates them behind the
        # embeddings); LinearGroupOp then forms the input gradient for those columns only
        self.grad_cols = 0
        # operand magnitudes for the two-plane fp16 GEMMs (include/mmlrec.h): slot of the value, slot of its gradient,
        # and how many of the gradient's writers raised that slot (valid iff it equals `written`)
        self.amax = None
        self.gamax = None
        self.gamax_writers = 0
        # bf16-storage path (include/mmlrec.h K3'): the value lives in a bf16 buffer -- only GEMMs read it; producer16:
        # a bf16-storage layer group produced it and will read its GRADIENT as a GEMM operand (Plan.grad_of)
        self.producer16 = False

    @property
    def is16(self):
        return self.buf.dtype == torch.bfloat16

    @property
    def n(self):
        return self.buf.shape[1]


INLINE = object()  # call-list marker: (INLINE, python_callable, args) run in place like a PY entry but do NOT cut a HIP graph
# (stream fork / join of trainer.InnerFork: event record / wait, capturable)
PY = object()  # call-list marker: (PY, python_callable, args[, meta]) entries (collectives) next to (c_fn, args[, meta])


def call_meta(c):
    """The meta dict of a call-list entry -- (fn, args[, meta]), (PY, callable, args[, meta]) or (INLINE, callable, args) --
    or {} when the entry carries none.  The dict itself: a caller may mutate it in place (Plan.finish: `ready`)."""
    return c[-1] if isinstance(c[-1], dict) else {}


def has_py(calls):
    """Whether a call list holds a Python-issued entry (such a list is no single HIP graph: trainer.Segments cuts there)."""
    return any(c[0] is PY for c in calls)


def _claim(x):
    acc = 1 if x.written else 0
    x.written += 1
    return acc


@dataclasses.dataclass(frozen=True)
class PlanKnobs:
    """Every environment switch the recorder and the passes read, read ONCE per Plan (from_env; never at import: tests and
    lab scripts set the variables between constructions) and kept as plan.knobs.  The A/B behind a switch stands where
    the switch is used.  MMLREC_DEFER_REDUCE is not here: it overrides a context, not a plan (_defer_reduce)."""
    amax: typing.Optional[bool] = None  # MMLREC_AMAX=0 / 1: the two-plane fp16 GEMMs off / on; unset: from B = 32 768 on
    bf16_storage: bool = True    # MMLREC_BF16_STORAGE=0: fp32 buffers under GEMM mode 1 too (operands rounded in registers)
    gemm_planes: bool = True     # MMLREC_GEMM_PLANES=0: no pre-cut weight planes, every wave cuts the fragment it stages
    merge_copies: bool = True    # MMLREC_MERGE_COPIES=0: neighbouring strided copies stay one launch each
    amax_merge: bool = True      # MMLREC_AMAX_MERGE=0: the weights' magnitudes in a launch of their own (round 3)
    nt_group: int = L.NT_MAX_GROUP  # MMLREC_NT_GROUP=n: problems per merged gemm_nt_kernel launch (16: round 5's launches)
    tower_head: bool = True      # MMLREC_TOWER_HEAD=0: last tower layer, heads and the towers' dgrad stay three launches
    gather_wgmax: bool = True    # MMLREC_GATHER_WGMAX=0: the gathered input's magnitude from a pass over the whole output
    det_fused: bool = True       # MMLREC_DET_FUSED=0: the deterministic scatter measures and finalizes for itself
    grad_parts: bool = True      # MMLREC_GRAD_PARTS=0: gate products that share a factor accumulate into ONE buffer, in order
    grad_cols: bool = True       # MMLREC_GRAD_COLS=0: the input gradient is formed for every column, read or not
    split_dgrad: bool = True     # MMLREC_SPLIT_DGRAD=0: a many-source input gradient stays ONE problem at small batches

    @classmethod
    def from_env(cls, env=None):
        env = os.environ if env is None else env

        def on(name):
            return env.get(name, "1") != "0"

        return cls(amax={"0": False, "1": True}.get(env.get("MMLREC_AMAX", "")),
                   bf16_storage=on("MMLREC_BF16_STORAGE"), gemm_planes=on("MMLREC_GEMM_PLANES"),
                   merge_copies=on("MMLREC_MERGE_COPIES"), amax_merge=on("MMLREC_AMAX_MERGE"),
                   nt_group=min(L.NT_MAX_GROUP, max(1, int(env.get("MMLREC_NT_GROUP", str(L.NT_MAX_GROUP))))),
                   tower_head=on("MMLREC_TOWER_HEAD"), gather_wgmax=on("MMLREC_GATHER_WGMAX"),
                   det_fused=on("MMLREC_DET_FUSED"), grad_parts=on("MMLREC_GRAD_PARTS"), grad_cols=on("MMLREC_GRAD_COLS"),
                   split_dgrad=on("MMLREC_SPLIT_DGRAD"))


class Plan:
    def __init__(self, device, B, training, use_amax=None):
        self.device, self.B, self.training = device, int(B), bool(training)
        knobs = self.knobs = PlanKnobs.from_env()
        self.ops = []
        self.fwd, self.head_infer, self.head_train, self.head_bwd, self.bwd = [], [], [], [], []
        # backward is kept in three pieces so a trainer can overlap them on two HIP streams: `bwd` = the critical
        # chain (dgrads, gate/elementwise backward), `bwd_tail` = the table scatter (needs d(dnn_input), feeds the
        # HBM-bound table optimizer), `bwd_side` = every weight-gradient GEMM (MFMA-bound, needs only values the
        # chain has already produced).  Sequential order bwd -> bwd_tail -> bwd_side is always valid.
        self.bwd_tail, self.bwd_side = [], []
        self.head_side = []  # the deferred reduction of the fused head call (dw / dbias / loss): beside `bwd_side`
        self.keep = []  # ctypes descriptor blocks + buffers referenced by raw pointer
        # dropout (DropoutOp): on iff the MODULE is in training mode; the step word of its mask stream is read from
        # `step_dev` (the optimizer's device step counter when the model has one, else a counter of the plan's own)
        self.dropout_on = False
        self.row0 = 0  # first row of this plan's batch in the global batch (data-parallel ranks: rank * B)
        self.dropout_seed = 0
        self.step_dev = None
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.vals = {}
        self.prob = None
        self.loss = torch.zeros(1, dtype=torch.float32, device=device)
        self.y = None
        self.mask = None
        self.dprob = None
        self.X = None
        self.layer_outputs = {}
        # operand magnitudes (ops.amax_slots): one pool per plan, zeroed at the start of every forward; the magnitudes of
        # the stable weights are measured by ONE launch right after (amax_pre, put in front of `fwd` by finish())
        # Large batches: the GEMMs are throughput-bound and the two-plane fp16 form pays (AE-30 at 65 536: GEMM family
        # 1.14 -> 1.0 ms, step -5 %).  Same-box A/B at smaller batches: level at 32 768 and 16 384 (+-2 %: the ~50 us of
        # magnitude launches per step against the arithmetic saved), a loss below (8 192: 0.839 -> 0.854 ms; lazy_exact at
        # 4 096: 0.27 -> 0.35 ms -- a step there is a chain of ~25 short launches).  With the cheaper cut and the pre-cut
        # weights of the end of round 3: 32 768: 1.272 -> 1.244 ms (lazy_exact 0.927 -> 0.894), 16 384: 0.994 -> 1.036,
        # 8 192: 0.760 -> 0.802, 4 096: 0.696 -> 0.720.  So: on from 32 768 samples per step, the three-plane bf16 form
        # below.  MMLREC_AMAX=0 / 1 forces.
        self.use_amax = knobs.amax if knobs.amax is not None else self.B >= 32768
        if use_amax is False:
            # (a PCGrad per-task plan replays its backward once per objective: the gradient slots only ever rise within a
            # step, so a later pass would cut its operands with an earlier pass's magnitudes)
            self.use_amax = False
        self.pcgrad_T = 0  # > 0: the plan of a PCGrad per-task step (trainer.PCGradSchedule) over that many objectives
        # bf16-STORAGE path (round 5, include/mmlrec.h K3'; BASELINE.json configs[1]): under the opt-in reduced-precision
        # GEMM mode 1 (operands rounded to bf16) the values and gradients that only GEMMs read are STORED as bf16 and the
        # layer groups that read them run csrc/gemm16.hip -- same products, half the activation traffic, no conversion in
        # the kernels.  Models mark such values (Plan.val(store16=True)); MMLREC_BF16_STORAGE=0 keeps fp32 buffers.
        self.bf16 = (device.type == "cuda" and knobs.bf16_storage and
                     L.load().mml_gemm_get_mode() == 1)
        if self.bf16:
            self.use_amax = False  # (mode 1 reads no operand magnitudes)
        # the mml_tower_head_group of the fused top of the network (passes.fuse_tower_head), if any: such a plan's `fwd` no
        # longer writes the heads' input, so only run_train_fwd_bwd replays it (_refuse_fused)
        self.tower_head = None
        self.cast16_items = []   # (fp32 weight, bf16 copy, transposed): refreshed by ONE launch at the start of a step
        self.cast16_cache = {}
        self.amax_pool = ops.amax_slots(1024, device) if (device.type == "cuda" and self.use_amax) else None
        self.amax_next = 0
        self.amax_weights = {}   # (data_ptr, shape) -> slot
        self.amax_wlist = []     # (tensor, slot) of the stable weights
        # pre-cut weights (mml_gemm_planes_cut): the two fp16 planes of every stable weight the forward / input-gradient
        # GEMMs read, cut once at the start of a step instead of by every wave that stages a fragment of it
        self.planes_items = []   # (W, planes, layout, [slots], kexp)
        self.planes_cache = {}
        self.n_pre = 0           # entries of `fwd` that precede the first op's calls (prepend)
        self.amax_pre_done = self.cast16_pre_done = False  # passes.amax_prologue / cast16_prologue ran

    # ---- buffers -----------------------------------------------------------------------------
    def empty(self, *shape, dtype=torch.float32):
        t = torch.empty(*shape, dtype=dtype, device=self.device)
        self.keep.append(t)
        return t

    def zeros(self, *shape, dtype=torch.float32):
        t = torch.zeros(*shape, dtype=dtype, device=self.device)
        self.keep.append(t)
        return t

    def workspace(self, nbytes, least=4):
        """A kept uint8 buffer of max(nbytes, least) bytes: the workspace of ONE recorded call (never the shared scratch)."""
        ws = torch.empty(max(int(nbytes), least), dtype=torch.uint8, device=self.device)
        self.keep.append(ws)
        return ws

    def bound(self, b, **meta):
        """The call-list entry (fn, args, meta) of a bind.Bound; the ctypes arrays and descriptors among its arguments
        are kept alive with the plan."""
        self.keep += [getattr(a, "_obj", a) for a in b.args
                      if isinstance(getattr(a, "_obj", a), (C.Array, C.Structure))]
        return (getattr(L.load(), b.name), b.args, meta)

    def _rows(self, n, pad_k=False):
        """[B, n] view of a fresh buffer with 16-byte aligned rows.  pad_k: when n is not a multiple of 16 the row is
        padded with ZERO columns up to the next multiple (returns the padded width, else 0)."""
        if pad_k and n % 16:
            kp = (n + 15) // 16 * 16
            return self.zeros(self.B, kp)[:, :n], kp
        ld = (n + 3) // 4 * 4
        return (self.empty(self.B, ld)[:, :n] if ld != n else self.empty(self.B, n)), 0

    def val(self, n, act=L.ACT_NONE, needs_grad=True, name="", buf=None, pad_k=False, store16=False):
        """pad_k: for values that feed a GEMM as the reduction operand (see Val.kpad).  store16: the value is read by
        bf16-storage layer groups ONLY (the caller vouches for it; finish() checks) -- a bf16 buffer when the plan runs
        the bf16-storage path."""
        kp = 0
        if buf is None:
            if store16 and self.bf16 and n % 8 == 0:
                buf = self.empty(self.B, n, dtype=torch.bfloat16)
            else:
                buf, kp = self._rows(n, pad_k)
        v = Val(buf, act, needs_grad, name)
        v.kpad = kp
        return v

    def _grad16(self, v):
        """dL/dv as a bf16 buffer: a bf16-storage layer group produced v (it reads the gradient as a GEMM operand), and v's
        one consumer writes the gradient exactly once, in bf16."""
        return (self.bf16 and v.producer16 and v.n % 8 == 0 and len(v.consumers) == 1 and
                v.consumers[0].writes_grad16(self, v))

    def weight16(self, pv, transposed):
        """bf16 copy of a weight ([N, K], or transposed [K, N]: the input gradient reads W^T rows), refreshed by the
        cast launch that opens the step."""
        key = (pv.data.data_ptr(), tuple(pv.data.shape), bool(transposed))
        if key not in self.cast16_cache:
            W = pv.data
            if W.dim() != 2 or W.stride(1) != 1:
                raise L.MMLError("bf16-storage path: 2-D weights with unit inner stride")
            shape = (W.shape[1], W.shape[0]) if transposed else tuple(W.shape)
            dst = torch.zeros(shape, dtype=torch.bfloat16, device=self.device)
            self.cast16_cache[key] = dst
            self.cast16_items.append((W, dst, bool(transposed)))
        return self.cast16_cache[key]

    def grad_of(self, v):
        """Allocate v.grad on first use (same row pitch as the value)."""
        if v.grad is None:
            if self._grad16(v):
                v.grad = self.empty(self.B, v.n, dtype=torch.bfloat16)
            elif v.is16:  # (a bf16 value whose gradient is fp32: the gather's output -- the table scatter reads it)
                v.grad = self.empty(self.B, v.n)
            elif v.kpad:
                v.grad = self.zeros(self.B, v.kpad)[:, :v.n]
            else:
                ld = (v.n + 3) // 4 * 4
                v.grad = self.empty(self.B, ld)[:, :v.n] if ld != v.n else self.empty(self.B, v.n)
        return v.grad

    # ---- operand magnitudes --------------------------------------------------------------------
    def new_amax(self):
        if self.amax_pool is None:
            return None
        if self.amax_next >= self.amax_pool.shape[0]:
            raise L.MMLError("operand-magnitude pool exhausted")
        self.amax_next += 1
        return self.amax_pool[self.amax_next - 1]

    def weight_amax(self, pv, tensor, need):
        """Slot of a GEMM weight operand.  `tensor` may be a zero-padded copy of pv.data (same magnitude).  Stable
        parameters join the start-of-step launch; anything else is appended to `need` (measured before the launch that
        is being recorded)."""
        if self.amax_pool is None:
            return None
        key = (pv.data.data_ptr(), tuple(pv.data.shape))
        if key in self.amax_weights:
            return self.amax_weights[key]
        slot = self.new_amax()
        if getattr(pv, "stable", False):
            self.amax_weights[key] = slot
            self.amax_wlist.append((pv.data, slot))
        else:
            need.append((pv.data, slot))  # (not cached: re-measured by every launch that reads it -- it may change)
        return slot

    def weight_planes(self, q, layout, group=None, padded=False):
        """(planes, kexp) of problem q's weight for the forward (layout ROWS: its own exponent) or as one source of an
        input-gradient problem (layout COLS: `group` = the problems whose weights feed the same output, ONE exponent), or
        (None, None): only stable weights in nn.Linear layout whose magnitude is taken at the start of the step.
        padded: the launch reads the zero-padded operand (q["Wp"], reduction extent rounded up to 16): the planes are cut
        from the weight itself into a zero-initialised buffer of the padded shape."""
        if self.amax_pool is None or not self.knobs.gemm_planes:
            return None, None
        qs = [q] if group is None else group
        slots = []
        # K6: a derived weight W = A (.) B whose factors are stable parameters (STAR: W_specific (.) W_shared, reference
        # model/utils.py:214-218) is cut straight from its factors; all members of a group must be of one kind
        prod = [getattr(g["W"], "factors", None) is not None for g in qs]
        if any(prod) and not all(prod):
            return None, None
        for g in qs:
            W = g["W"]
            kn = int(g.get("w_kn", 0))
            # a [K, N] matrix (w_kn = 1) swaps the roles: the forward's reduction runs down its rows
            lay = layout if not kn else (ops.PLANES_COLS if layout == ops.PLANES_ROWS else ops.PLANES_ROWS)
            red = W.data.shape[1] if lay == ops.PLANES_ROWS else W.data.shape[0]
            if (("Wp" in g) != bool(padded) or W.data.dim() != 2 or W.data.stride(1) != 1 or
                    (red % 16 and not (padded and lay == ops.PLANES_ROWS)) or
                    W.data.data_ptr() % 16 or (W.data.stride(0) % 4 and not padded)):
                return None, None
            fac = getattr(W, "factors", None)
            if fac is not None:
                if padded or not all(getattr(f, "stable", False) and f.data.shape == W.data.shape and
                                     f.data.stride(1) == 1 for f in fac):
                    return None, None
                sl = tuple(self.weight_amax(f, f.data, None) for f in fac)  # (stable: the start-of-step launch)
                slots.append(sl)
                continue
            key = (W.data.data_ptr(), tuple(W.data.shape))
            if kn or not getattr(W, "stable", False) or key not in self.amax_weights:
                return None, None
            slots.append(self.amax_weights[key])
        if any(prod) and 2 * len(slots) > L.MAX_SRC:
            return None, None
        Wq = q["W"]
        W = Wq.data
        kn = int(q.get("w_kn", 0))
        lay = layout if not kn else (ops.PLANES_COLS if layout == ops.PLANES_ROWS else ops.PLANES_ROWS)
        shape = tuple(q["Wp"].shape) if padded else (W.shape[0], W.stride(0))
        flat = tuple(s_.data_ptr() for sl in slots for s_ in (sl if isinstance(sl, tuple) else (sl,)))
        ck = (W.data_ptr(), tuple(W.shape), lay, bool(padded), flat)
        if ck not in self.planes_cache:
            gk = ("kexp", lay, bool(padded), flat)  # one exponent word per group
            if gk not in self.planes_cache:
                self.planes_cache[gk] = torch.zeros(1, dtype=torch.int32, device=self.device)
            planes = torch.zeros(shape, dtype=torch.int32, device=self.device)
            if not padded:
                planes = planes[:, :W.shape[1]]
            self.planes_cache[ck] = (planes, self.planes_cache[gk])
            src = W if not any(prod) else tuple(f.data for f in Wq.factors)
            self.planes_items.append((src, planes, lay, slots, self.planes_cache[gk]))
        return self.planes_cache[ck]

    def value_amax(self, v, view, need):
        """Slot of a forward value used as a GEMM operand: the producer's, or measured now (once)."""
        if self.amax_pool is None:
            return None
        if v.amax is None:
            v.amax = self.new_amax()
            # (a producer may have left partial maxima of the whole value: a bound of any view of it)
            src = getattr(v, "amax_src", None)
            need.append((src if src is not None else view, v.amax))
        return v.amax

    def raised_grad_slot(self, v):
        """v's gradient slot if every writer of v.grad recorded so far raised it (grad_slot / shared_grad_slot), else None."""
        return v.gamax if (v.gamax is not None and v.gamax_writers == v.written and v.written > 0) else None

    def grad_amax(self, v, need):
        """Slot of v.grad as a GEMM operand, called when every writer of the gradient has been recorded: the slot the
        writers raised if ALL of them did, else measured now."""
        if self.amax_pool is None:
            return None
        if self.raised_grad_slot(v) is not None:
            return v.gamax
        v.gamax = self.new_amax()
        v.gamax_writers = v.written
        need.append((v.grad, v.gamax))
        return v.gamax

    def grad_slot(self, v):
        """The magnitude slot of v.grad that the launch being recorded must raise with what it stores, or None.  Called by a
        writer right after its _claim(v).  The slot stays valid for grad_amax as long as EVERY writer so far came through
        here: one that did not leaves the count behind, and neither it nor any later writer gets the slot."""
        if self.amax_pool is None:
            return None
        if v.gamax is None:
            v.gamax = self.new_amax()
        if v.gamax_writers != v.written - 1:
            return None
        v.gamax_writers += 1
        return v.gamax

    def shared_grad_slot(self, vals, slot=None):
        """ONE magnitude slot (`slot`, or a fresh one) for the gradients of all `vals`: the op that calls this has claimed
        each of them, is their only writer and raises the slot with every gradient it stores -- an upper bound for each."""
        if self.amax_pool is None:
            return None
        if slot is None:
            slot = self.new_amax()
        for v in vals:
            v.gamax, v.gamax_writers = slot, v.written
        return slot

    def amax_call(self, need, lib=None, **meta):
        arr = ops.make_amax_descs(need)
        self.keep.append(arr)
        m = dict(kernel="amax_kernel", bytes=4.0 * sum(t.numel() for t, _ in need), need=list(need))
        m.update(meta)
        return ((lib or L.load()).mml_amax_batch, (arr, len(need)), m)

    # ---- execution ---------------------------------------------------------------------------
    @staticmethod
    def _run(calls):
        s = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else None
        if profiling.enabled:  # --profile: one roctx range per call, named after its kernel
            for c in calls:
                if c[0] is INLINE:  # (stream fork / join: the calls it issues open their own ranges)
                    c[1](*c[2])
                    continue
                with profiling.range(call_meta(c).get("kernel") or getattr(c[1] if c[0] is PY else c[0], "__name__", "call")):
                    if c[0] is PY:
                        c[1](*c[2])
                    else:
                        rc = c[0](*c[1], s)
                        if rc:
                            L.check(rc, c[0].__name__)
            return
        for c in calls:
            if c[0] is PY or c[0] is INLINE:
                c[1](*c[2])
                continue
            rc = c[0](*c[1], s)
            if rc:
                L.check(rc, c[0].__name__)

    @staticmethod
    def run_timed(calls, acc):
        """Diagnostic replay: brackets every C-ABI call with HIP events on the launch stream and adds
        (milliseconds, launches) per call label into `acc` (used by bench.py for the roofline line)."""
        s = torch.cuda.current_stream()
        evs = []
        for c in calls:
            if c[0] is INLINE:  # (stream fork / join: run in place, untimed -- what it issues is not this stream's time)
                c[1](*c[2])
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            if c[0] is PY:
                c[1](*c[2])
            else:
                rc = c[0](*c[1], s.cuda_stream)
                if rc:
                    L.check(rc, c[0].__name__)
            b.record(s)
            label = None
            if c[0] is not PY and str(call_meta(c).get("kernel", "")).startswith("gemm<"):
                label = L.load().mml_gemm_last_kernel().decode() or None
            evs.append((c, a, b, label))
        torch.cuda.synchronize()
        for c, a, b, label in evs:
            meta = call_meta(c) or {"kernel": getattr(c[1], "__name__", "python") if c[0] is PY else c[0].__name__}
            e = acc.setdefault(label or meta["kernel"], {"ms": 0.0, "launches": 0, "flops": 0.0, "bytes": 0.0,
                                                         "hbm_bytes": 0.0})
            e["ms"] += a.elapsed_time(b)
            e["launches"] += 1
            e["flops"] += meta.get("flops", 0.0)
            e["bytes"] += meta.get("bytes", 0.0)
            # compulsory HBM bytes of the call (every distinct operand read once, every output written once): the GEMM
            # launches are priced in FLOPs (`flops`) but still move their operands -- bench.py's whole-step fraction
            e["hbm_bytes"] = e.get("hbm_bytes", 0.0) + meta.get("hbm_bytes", meta.get("bytes", 0.0))

    def _refuse_fused(self, what):
        if self.tower_head is not None:
            raise L.MMLError(f"{what} on a plan rewritten by fuse_tower_head: its forward no longer stores the heads' "
                             "input, which this entry point reads (run_train_fwd_bwd replays such a plan)")

    def run_forward(self):
        self._refuse_fused("run_forward")
        self._run(self.fwd)
        self._run(self.head_infer)

    def run_train_fwd_bwd(self):
        """forward + summed-BCE loss + backward (gradients land in the PVal.grad buffers)."""
        self._run(self.fwd)
        self._run(self.head_train)
        self._run(self.bwd)
        self._run(self.bwd_tail)
        self._run(self.head_side)
        self._run(self.bwd_side)

    def run_backward_from_dprob(self):
        self._refuse_fused("run_backward_from_dprob")
        self._run(self.head_bwd)
        self._run(self.bwd)
        self._run(self.bwd_tail)
        self._run(self.bwd_side)

    # ---- graph recording ---------------------------------------------------------------------
    def prepend(self, calls):
        """Puts `calls` in front of `fwd`: the ONE way entries get there (the prologues of passes.py, the step counter of an
        uncompiled model with dropout), so n_pre counts them all -- trainer.segmented_step cuts the forward by it."""
        self.fwd[:0] = calls
        self.n_pre += len(calls)

    def add(self, op):
        self.ops.append(op)
        seen = set()
        for v in op.inputs():
            if isinstance(v, Val) and v.needs_grad and id(v) not in seen:
                seen.add(id(v))
                v.consumers.append(op)
        self.fwd.extend(op.fwd_calls(self))
        return op

    def finish(self, head_op):
        """Record the head op and derive the backward call list."""
        self.head_op = head_op
        for v in head_op.inputs():
            if isinstance(v, Val) and v.needs_grad:
                v.consumers.append(head_op)
        self.head_infer = head_op.infer_calls(self)
        from . import passes  # (passes imports this module)
        if not self.training:
            passes.amax_prologue(self)
            passes.cast16_prologue(self)
            return
        calls = head_op.train_calls(self, use_dprob=False)
        self.head_train = [c for c in calls if not call_meta(c).get("side")]
        # (belongs to head_train, not to the backward every path shares: run_backward_from_dprob has its own head call)
        self.head_side = [c for c in calls if call_meta(c).get("side")]
        self.head_bwd = head_op.train_calls(self, use_dprob=True, claim=False)
        for op in reversed(self.ops):
            for v in op.outputs():
                if isinstance(v, Val) and v.grad is not None and v.act != L.ACT_NONE and not v.deriv_applied:
                    if v.is16 or v.grad.dtype != torch.float32:
                        raise L.MMLError(f"bf16 value {v.name!r}: its activation derivative must fold into its one consumer")
                    self.bwd.append(self.bound(bind.act_bwd(v.buf, v.grad, v.grad, v.act, n=self._flat_numel(v))))
                    v.deriv_applied = True
            mine = []
            for c in op.bwd_calls(self):
                meta = call_meta(c)
                if meta.get("side"):
                    self.bwd_side.append(c)
                    mine.append(c)
                elif meta.get("tail"):
                    self.bwd_tail.append(c)
                else:
                    self.bwd.append(c)
            # a side call reads dL/d(this op's outputs) and forward values only: it may start once the chain has issued
            # everything up to and including this op's own entries (TrainStep's early fork of the side stream)
            for c in mine:
                call_meta(c)["ready"] = len(self.bwd)  # (an index into `bwd`: passes.reindex_ready)
        passes.amax_prologue(self)
        passes.cast16_prologue(self)
        passes.merge_plan_copies(self)
        # (Measured on MI355X: issuing every weight-gradient partial-product GEMM before the first reduction -- the
        # phased wgrad entry point allows it -- makes the step SLOWER, 2.35 ms vs 2.19 ms: the GEMMs then run next to
        # the table scatter and the dense table optimizer for longer and all of them are HBM-bound together.  The
        # list stays in program order: partial products and reduction of one layer back to back.)

    def _flat_numel(self, v):
        # act_bwd is a flat kernel: value and gradient must share the padded pitch (they do by construction)
        if v.buf.stride(0) != v.grad.stride(0):
            raise L.MMLError("value / gradient pitch mismatch for " + v.name)
        if v.buf.stride(0) != v.n and v.buf.storage_offset() % v.buf.stride(0) != 0:
            raise L.MMLError("cannot finalise a column-sliced value: " + v.name)
        return self.B * v.buf.stride(0) if v.buf.stride(0) != v.n else self.B * v.n


# ==================================================================================================
# ops
# ==================================================================================================
def _distinct_bytes(tensors):
    """Bytes of the distinct buffers among `tensors` (torch tensors / None; a view counts its own elements)."""
    seen, n = set(), 0
    for t in tensors:
        if t is None:
            continue
        key = (t.data_ptr(), tuple(t.shape))
        if key not in seen:
            seen.add(key)
            n += t.numel() * t.element_size()
    return float(n)


def _gemm_symbol(arc, brc, cols, epi, kreds=(), tensors=(), nrc_extents=()):
    """Provisional label of a grouped GEMM launch; Plan.run_timed replaces it with the symbol the C side actually
    launched (mml_gemm_last_kernel), which depends on the tile / arithmetic choice made in csrc/gemm.hip."""
    return "gemm<%s>" % ("fwd", "dgrad", "wgrad")[epi]


def scatter_symbol(E):
    """Kernel symbol of a scatter / index-unique launch (csrc/gather_scatter.hip: scatter_impl's choice)."""
    return "scatter_fold_kernel" if E in (4, 8, 16) else ("scatter_hash_kernel" if E <= 16 else "scatter_atomic_kernel")


class Op:
    def writes_grad16(self, plan, v):
        """bf16-storage path: this op, as the ONLY consumer of v, writes dL/dv once and can write it as bf16."""
        return False

    def inputs(self):
        return []

    def outputs(self):
        return []

    def fwd_calls(self, plan):
        return []

    def bwd_calls(self, plan):
        return []


class GatherOp(Op):
    """K1/K2: multi-field gather (+dense copy) and its scatter backward."""

    def __init__(self, tables, X, cols, dense_col0, nd, out, sparse_rows=None):
        self.tables, self.X, self.cols, self.dense_col0, self.nd, self.out = tables, X, cols, dense_col0, nd, out
        self.sparse_rows = sparse_rows  # TableRows bookkeeping (seen bitmaps, touched list) or None
        self.mark_rows = None  # TableRows: the forward marks the rows it reads and lists them (split dense update)
        # uint8 map (ops.marks_bytes layout): the scatter marks every row it adds to, the dense table optimizer skips
        # the gradient read of unmarked rows and clears the marks (mml_opt_tensor.grad_marks)
        self.grad_marks = None
        # True: the backward is mml_scatter_bwd_det -- order-independent integer fixed-point sums, bitwise repeatable
        # (BaseModel.scatter_mode = "deterministic"); needs store.ensure_det(tables)
        self.deterministic = None
        # set by bwd_calls when the deterministic scatter leaves its 64-bit row totals to the table optimizer
        # (MML_SCATTER_DET_DEFER_TOTALS): dict(slot, shift) that optimizer.Optimizer hands to mml_opt_tensor
        self.det_deferred = None

    def outputs(self):
        return [self.out]

    def index_view(self, plan):
        """(index matrix, rows) the table update of this step is built from (the global batch under replication)."""
        return self.X, plan.B

    def pre_index_calls(self, plan):
        return []

    def fwd_calls(self, plan):
        F = len(self.tables)
        E = self.tables[0].data.shape[1]
        # (tables, X, cols, dense_col0, nd): how every bind.gather* builder opens
        src = ([t.data for t in self.tables], self.X, self.cols, self.dense_col0, self.nd)
        meta = dict(kernel="gather_vec4_kernel" if E % 4 == 0 else "gather_scalar_kernel",
                    bytes=float(plan.B) * (F * (4 + 8 * E) + 8 * self.nd))  # index + row read + row write
        mr = self.mark_rows
        out = self.out.buf
        if self.out.is16:  # bf16-storage path: dnn_input leaves the gather as the first layers' GEMM operand
            if mr is not None:
                raise L.MMLError("the row-marking gather has no bf16 form (split dense update)")
            return [plan.bound(bind.gather16_fwd(*src, out, plan.status, B=plan.B), kernel="gather16_kernel",
                               bytes=float(plan.B) * (F * (4 + 6 * E) + 6 * self.nd))]
        if mr is not None:
            return [plan.bound(bind.gather_fwd_mark(*src, out, mr.marks, plan.status, B=plan.B), **meta),
                    plan.bound(bind.rows_compact([t.data.shape[0] for t in self.tables], bind.rows_args(mr)),
                               kernel="rows_compact_kernel", bytes=float(mr.marks.numel()))]
        nwg = int(L.load().mml_gather_wgmax_len(F, E, self.nd, plan.B)) if plan.amax_pool is not None else 0
        if (nwg > 0 and plan.knobs.gather_wgmax and ops._ld(out) % 4 == 0 and
                out.data_ptr() % 16 == 0 and all(t.data.data_ptr() % 16 == 0 for t in self.tables)):
            # the magnitude of the gathered input comes out of the gather itself: one value per workgroup, read by the
            # magnitude launch in front of the first GEMM instead of a pass over the whole output (25 -> 6 us at 65 536)
            wg = plan.zeros(1, nwg)
            self.out.amax_src = wg
            return [plan.bound(bind.gather_fwd_wgmax(*src, out, wg, nwg, plan.status, B=plan.B), **meta)]
        return [plan.bound(bind.gather_fwd(*src, out, plan.status, B=plan.B), **meta)]

    def _det_setup(self, plan, emb_cols, shift):
        """The buffers and flags of the deterministic scatter call (mml_scatter_bwd_det / mml_scatter_pool_bwd_det):
        (mark map, magnitude slot, flags); sets self.det_deferred.  emb_cols: the columns of
        d(dnn_input) the scatter reads, shift: the totals' shift for this batch."""
        det, sr = self.deterministic, self.sparse_rows
        marks = self.grad_marks if self.grad_marks is not None else (sr.marks if sr is not None else det["marks"])
        keep_marks = self.grad_marks is not None or sr is not None
        slot = det["slot"]
        flags = 0 if keep_marks else L.SCATTER_DET_CLEAR_MARKS
        fused = plan.knobs.det_fused  # (MMLREC_DET_FUSED=0: the call measures and finalizes for itself)
        g = self.out
        # the magnitude of d(dnn_input) from the launch that wrote it: the one writer raised g.gamax (a slot of the
        # pool the step's opening mml_amax_reset zeroes) with the exact maximum over the [B, emb_cols] region read here
        if (fused and self.nd == 0 and getattr(g, "gamax_exact", False) and g.written == 1 and
                plan.raised_grad_slot(g) is not None and g.n == emb_cols):
            slot = g.gamax
            flags |= L.SCATTER_DET_AMAX_SUPPLIED
        # the totals stay in acc64 for the ONE marked streaming launch of the dense table optimizer
        self.det_deferred = None
        # (never in a PCGrad per-task plan: its banks take the fp32 rows of every pass; never in the multi-GPU subclasses)
        if (fused and type(self) in (GatherOp, PooledGatherOp) and sr is None and not getattr(plan, "pcgrad_T", 0) and
                L.opt_takes_det_totals([t.data.numel() for t in self.tables], self.grad_marks is not None)):
            flags |= L.SCATTER_DET_DEFER_TOTALS
            self.det_deferred = dict(slot=slot, shift=shift)
        return marks, slot, flags

    def _rows_args(self):
        """The touched-row arguments of the scatter call: the bookkeeping of self.sparse_rows (one entry per table), or
        the marks alone."""
        return bind.rows_args(self.sparse_rows, marks=self.grad_marks)

    def _compact_entry(self, plan):
        """The compaction behind a deterministic scatter: the marks it left -> the touched list of self.sparse_rows."""
        return plan.bound(bind.rows_compact([t.data.shape[0] for t in self.tables], self._rows_args()),
                          kernel="rows_compact_kernel", bytes=float(self.sparse_rows.marks.numel()), tail=True)

    def bwd_calls(self, plan):
        if self.out.grad is None or not any(t.needs_grad for t in self.tables):
            return []
        F = len(self.tables)
        E = self.tables[0].data.shape[1]
        gt = [t.grad for t in self.tables]
        for t in self.tables:
            _claim(t)
        meta = dict(kernel=scatter_symbol(E),
                    bytes=float(plan.B) * F * (4 + 12 * E), tail=True)  # idx + grad read + row RMW
        det = self.deterministic
        if det is not None:
            # deterministic scatter: 64-bit integer row totals, then fp32 (two launches + the magnitude of d(dnn_input),
            # or the fold alone: MML_SCATTER_DET_AMAX_SUPPLIED / _DEFER_TOTALS below);
            # the marks feed the marked dense update (left set) or the touched-row list (compaction, which clears them)
            marks, slot, flags = self._det_setup(plan, F * E, int(L.load().mml_scatter_det_shift(plan.B)))
            calls = [plan.bound(bind.scatter_bwd_det(gt, self.X, self.cols, self.out.grad, det["acc64"], slot, marks, flags,
                                                     plan.status, B=plan.B),
                                **dict(meta, kernel="scatter_fold_kernel<det>", det_flags=flags,
                                       ptrs=[a.data_ptr() for a in det["acc64"]]))]
            if self.sparse_rows is not None:
                calls.append(self._compact_entry(plan))
            return calls
        return [plan.bound(bind.scatter_bwd(gt, self.X, self.cols, self.out.grad, self._rows_args(), plan.status, B=plan.B),
                           **meta)]


class PooledGatherOp(GatherOp):
    """K1p / K2p: the gather of a schema with multi-valued (pooled) fields and its scatter backward.  `tables` holds
    every TABLE once (the order of optimizer.ParamStore.table_names, which is also the order of the touched-row bookkeeping);
    `singles` = [(X column, table number)], `pooled` = [(first X column, maxlen, combiner, table number, length column
    or None)] (model.utils.pooled_layout)."""

    def __init__(self, tables, X, singles, pooled, dense_col0, nd, out, sparse_rows=None):
        super().__init__(tables, X, None, dense_col0, nd, out, sparse_rows=sparse_rows)
        self.singles, self.pooled = list(singles), list(pooled)
        self.argmax = None

    def _desc(self, which):
        return ops.make_pool_desc([getattr(t, which) for t in self.tables], self.singles,
                                  [ops.PooledField(*pf) for pf in self.pooled])

    def _lookups(self):
        return len(self.singles) + sum(pf[1] for pf in self.pooled)

    def fwd_calls(self, plan):
        if self.out.is16 or self.mark_rows is not None:
            raise L.MMLError("the pooled gather has no bf16-storage form and no row-marking form")
        E, P = self.tables[0].data.shape[1], len(self.pooled)
        d = self._desc("data")
        if any(pf[2] == "max" for pf in self.pooled):
            self.argmax = plan.zeros(plan.B, P * E, dtype=torch.uint8)
        # ids + rows read (every position: an upper bound of the valid ones) + blocks and dense columns written
        meta = dict(kernel="gather_pool_kernel",
                    bytes=float(plan.B) * (len(self.singles) * (4 + 8 * E) + 8 * self.nd +
                                           sum(4 * pf[1] + 4 * E * pf[1] + 4 * E for pf in self.pooled)))
        wg, nwg = None, 0
        if plan.amax_pool is not None and plan.knobs.gather_wgmax:
            nwg = int(L.load().mml_gather_pool_wgmax_len(C.byref(d), self.nd, plan.B))
            if nwg > 0:
                wg = plan.zeros(1, nwg)
                self.out.amax_src = wg
        return [plan.bound(bind.gather_pool_fwd(d, self.X, self.dense_col0, self.nd, self.out.buf, self.argmax, wg, nwg,
                                                plan.status, B=plan.B), **meta)]

    def bwd_calls(self, plan):
        if self.out.grad is None or not any(t.needs_grad for t in self.tables):
            return []
        E = self.tables[0].data.shape[1]
        d = self._desc("grad")
        for t in self.tables:
            _claim(t)
        meta = dict(kernel="scatter_pool_fold_kernel", tail=True,  # ids + dOut block read + row read-modify-write
                    bytes=float(plan.B) * (len(self.singles) * (4 + 12 * E) +
                                           sum(4 * pf[1] + 4 * E + 8 * E * pf[1] for pf in self.pooled)))
        det = self.deterministic
        if det is not None:
            # deterministic scatter (GatherOp.bwd_calls): totals, marks and the finalize launch are per TABLE
            shift = int(L.load().mml_scatter_pool_det_shift(C.byref(d), plan.B))
            if shift < 0:
                raise L.MMLError(f"deterministic pooled scatter: a batch of {plan.B} samples times the lookups of one "
                                 "table leaves no headroom in the 64-bit totals")
            marks, slot, flags = self._det_setup(plan, (len(self.singles) + len(self.pooled)) * E, shift)
            calls = [plan.bound(bind.scatter_pool_bwd_det(d, self.X, self.out.grad, self.argmax, det["acc64"], slot, marks,
                                                          flags, plan.status, B=plan.B),
                                **dict(meta, kernel="scatter_pool_fold_kernel<det>", det_flags=flags,
                                       ptrs=[a.data_ptr() for a in det["acc64"]]))]
            if self.sparse_rows is not None:
                calls.append(self._compact_entry(plan))
            return calls
        return [plan.bound(bind.scatter_pool_bwd(d, self.X, self.out.grad, self.argmax, self._rows_args(), plan.status,
                                                 B=plan.B), **meta)]

    def unique_calls(self, plan, rows):
        """The batch's distinct VALID rows per table -> `seen` bitmaps + touched list (the index pre-pass of lazy_exact)."""
        X, nrows = self.index_view(plan)
        return [plan.bound(bind.index_unique_pool(self._desc("data"), X, bind.rows_args(rows), plan.status, B=nrows),
                           kernel="mark_pool_rows_kernel+rows_compact_kernel", bytes=float(nrows) * self._lookups() * 5)]


def g16_layer_ok(B, K, N, training):
    """A Linear(K -> N) at batch B can run on the bf16-storage kernels (include/mmlrec.h K3': tile-aligned extents; the
    weight gradient's tiles are 128 x 128)."""
    ok = B % 128 == 0 and K % 64 == 0 and N % 64 == 0 and K > 0 and N > 0
    if training:
        ok = ok and K % 128 == 0 and N % 128 == 0
    return ok


def _fast_row_width_ok(n):
    return n % 4 == 0 and 0 < n <= 256  # (csrc/rows_route.hpp: head_route; the gate side asks gate_rows_shape)


def gate_rows_shape(H, gd_max, n_experts, n_gates, e_bf16):
    """Which fast gate kernels a group of this shape gets (L.GATE_SHAPE_* bits): the library's own rule under the process's
    switches (mml_gate_rows_shape, csrc/rows_route.hpp), asked before any buffer exists.  Only the fast kernels write or
    read bf16 tensors, so whoever chooses a storage format for a gate group's operands asks here."""
    return int(L.load().mml_gate_rows_shape(H, gd_max, n_experts, n_gates, int(bool(e_bf16))))


def _padded_view(buf, kp):
    """[B, kp] view over a value / gradient allocated by Plan._rows (columns [n, kp) are zero)."""
    if buf.stride(0) < kp or buf.stride(1) != 1:
        raise L.MMLError("value does not own zero-padded rows")
    return buf.as_strided((buf.shape[0], kp), (buf.stride(0), 1), buf.storage_offset())


def copy2d_descs(pairs, amax=None, accumulate=None):
    """The Copy2dDesc block of mml_copy2d_batch: src[:, :cols] -> dst[:, :cols] for every (src, dst) pair (cols = the narrower
    of the two).  amax: per pair a magnitude slot the copy raises with max |x| of what it stores, or None; accumulate: per
    pair whether the copy adds to dst instead of overwriting it (None = no pair does)."""
    arr = (L.Copy2dDesc * len(pairs))()
    for k, (d, (src, dst)) in enumerate(zip(arr, pairs)):
        d.src, d.lds, d.dst, d.ldd = src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0)
        d.rows, d.cols = src.shape[0], min(src.shape[1], dst.shape[1])
        d.accumulate = int(bool(accumulate[k])) if accumulate is not None else 0
        if amax is not None and amax[k] is not None:
            d.amax_out = amax[k].data_ptr()
    return arr


def _copy2d_batch_call(plan, pairs, amax=None, accumulate=None):
    """One launch of copy2d_descs(pairs, amax, accumulate); the plan keeps the block and the magnitude slots alive."""
    arr = copy2d_descs(pairs, amax, accumulate)
    plan.keep += [a for a in (amax or ()) if a is not None]
    plan.keep.append(arr)
    return (L.load().mml_copy2d_batch, (arr, len(pairs)),
            dict(kernel="copy2d_batch_kernel", bytes=8.0 * sum(min(a.numel(), b.numel()) for a, b in pairs)))


def _kpad_of(q):
    x = q["x"]
    if x.kpad and x.n % 16 and not q.get("w_kn", 0) and x.buf.stride(0) >= x.kpad:
        return x.kpad
    return 0


class LinearGroupOp(Op):
    """K3: a set of independent Linear(+activation) problems launched together.
    problems: dicts with x (Val), W (PVal), b (PVal or None), out (Val; out.act is the activation), w_kn.
    K7 (PepNet, reference model/pepnet.py:72-78, :139-140): a problem may also carry mul (Val) and prod (Val) -- the launch
    then stores prod = out * mul from the same epilogue (mml_gemm_fwd_desc.mul / prod), and the product's backward is
    folded into the input-gradient launch of the layer that READS prod (gate mode of mml_gemm_grouped_dgrad): neither
    direction makes a pass of its own over memory.  prod must feed exactly one LinearGroupOp."""

    def __init__(self, problems):
        self.p = problems
        self.use16 = False  # bf16-storage path (csrc/gemm16.hip): decided when the forward is recorded
        for q in self.p:
            # prod_bwd = "ext": only the FORWARD of the product rides in this launch's epilogue; its backward belongs to
            # another op (MulBatchOp(fwd_fused=True)) -- products no Linear layer reads (PepNet's gated input, the
            # products in front of the heads)
            if q.get("mul") is not None and q.get("prod_bwd") != "ext":
                q["prod"].gate = (q["mul"], q["out"])  # (h, g): factors of the product, for the consumer's dgrad

    def writes_grad16(self, plan, v):
        return self.use16 and v.is16

    # ---- bf16-storage path (include/mmlrec.h K3') --------------------------------------------------------------
    def _fwd16(self, plan):
        lib = L.load()
        probs = []
        for q in self.p:
            out = q["out"]
            if (not q["x"].is16 or q.get("w_kn") or q.get("mul") is not None or q["x"].kpad or
                    not g16_layer_ok(plan.B, q["x"].n, out.n, plan.training)):
                raise L.MMLError("bf16-storage layer group: every problem needs a bf16 input, a plain nn.Linear weight and "
                                 f"tile-aligned extents (got {q['x'].n} -> {out.n} at batch {plan.B})")
            if out.act not in (L.ACT_NONE, L.ACT_RELU):
                raise NotImplementedError("bf16-storage layer group: relu / linear activations")
            out.producer16 = True
            probs.append(dict(srcs=[(q["x"].buf, plan.weight16(q["W"], False))], C=out.buf,
                              bias=q["b"].data if q.get("b") else None, act=out.act,
                              mask_out=out.mask if out.act == L.ACT_RELU else None))
        calls = []
        for i in range(0, len(probs), L.G16_MAX_GROUP):
            ch, qs = probs[i:i + L.G16_MAX_GROUP], self.p[i:i + L.G16_MAX_GROUP]
            descs = ops.make_g16_tn_descs(ch)
            plan.keep.append(descs)
            meta = dict(kernel="g16_tn_kernel(fwd %dx%d->%d)" % (len(qs), qs[0]["x"].n, max(q["out"].n for q in qs)),
                        flops=sum(2.0 * plan.B * q["out"].n * q["x"].n for q in qs),
                        hbm_bytes=_distinct_bytes([q["x"].buf for q in qs] + [q["out"].buf for q in qs] +
                                                  [q["out"].mask for q in qs]) +
                        2.0 * sum(q["W"].data.numel() for q in qs))
            calls.append((lib.mml_g16_tn, (descs, len(ch)), meta))
        return calls

    def _casts16(self, plan, live):
        """The incoming gradients as bf16 operands (q["dC16"]): written that way by their producer (Plan.grad_of), else cast
        here, in ONE launch."""
        casts = []
        for q in live:
            g = q["out"].grad
            if g.dtype == torch.bfloat16:
                q["dC16"] = g
            else:
                if q["out"].act != L.ACT_NONE and not q["out"].deriv_applied:
                    raise L.MMLError("bf16-storage layer group: the activation derivative must be applied upstream")
                q["dC16"] = plan.empty(plan.B, q["out"].n, dtype=torch.bfloat16)
                casts.append((g, q["dC16"], False))
        if not casts:
            return []
        arr = ops.make_cast16_descs(casts)
        plan.keep.append(arr)
        return [(L.load().mml_cast16_batch, (arr, len(casts)),
                 dict(kernel="cast16_kernel", bytes=6.0 * sum(g.numel() for g, _, _ in casts)))]

    def _wgrad16_calls(self, plan, live):
        """Weight / bias gradients of the bf16-storage path (side list: only the optimizer reads them)."""
        lib = L.load()
        wg = []
        for q in live:
            if q["W"].needs_grad:
                acc, dbias = self._claim_wb(q)
                wg.append(dict(dC=q["dC16"], A=q["x"].buf, dW=q["W"].grad, dbias=dbias, accumulate=acc))
        calls = []
        for i in range(0, len(wg), L.G16_MAX_GROUP):
            ch = wg[i:i + L.G16_MAX_GROUP]
            descs = ops.make_g16_wgrad_descs(ch)
            nbytes = int(lib.mml_g16_wgrad_workspace_bytes(descs, len(ch)))
            if nbytes < 0:
                L.check(-1, "mml_g16_wgrad_workspace_bytes")
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=plan.device)
            plan.keep += [descs, ws]
            meta = dict(kernel="g16_nt_kernel(wgrad %dx%dx%d)" % (len(ch), ch[0]["dW"].shape[0], ch[0]["dW"].shape[1]),
                        flops=sum(2.0 * plan.B * q["dW"].numel() for q in ch), side=True,
                        rank=0, hbm_bytes=_distinct_bytes([q["dC"] for q in ch] + [q["A"] for q in ch] +
                                                          [q["dW"] for q in ch]))
            calls.append((lib.mml_g16_wgrad, (descs, len(ch), ws.data_ptr(), ws.numel(), 1), meta))
            calls.append((lib.mml_g16_wgrad, (descs, len(ch), ws.data_ptr(), ws.numel(), 2),
                          dict(kernel="g16_reduce_kernel", bytes=float(nbytes), side=True, rank=1)))
        return calls

    def _dgrad16_calls(self, plan, live):
        """Input gradients of the bf16-storage path: one problem per distinct input value, its layers as the sources."""
        dg = []
        for x, qs in self._by_input(live):
            if len(qs) > L.MAX_SRC:
                raise NotImplementedError("bf16-storage layer group: more than MAX_SRC layers on one input")
            plan.grad_of(x)
            fuse = len(x.consumers) == 1 and x.act == L.ACT_RELU and x.mask is not None
            if x.act != L.ACT_NONE and not fuse:
                raise L.MMLError(f"bf16 value {x.name!r}: its activation derivative must fold into its one consumer")
            acc = _claim(x)
            if acc and x.grad.dtype != torch.float32:
                raise L.MMLError("bf16 gradients cannot accumulate")
            dg.append((dict(srcs=[(q["dC16"], plan.weight16(q["W"], True)) for q in qs], C=x.grad, accumulate=acc,
                            mask_in=x.mask if fuse else None), x, qs))
            if fuse:
                x.deriv_applied = True
        calls = []
        for i in range(0, len(dg), L.G16_MAX_GROUP):
            ch = dg[i:i + L.G16_MAX_GROUP]
            descs = ops.make_g16_tn_descs([c[0] for c in ch])
            plan.keep.append(descs)
            meta = dict(kernel="g16_tn_kernel(dgrad %dx%d<-%d)" % (len(ch), ch[0][1].n, sum(q["out"].n for q in ch[0][2])),
                        flops=sum(2.0 * plan.B * x.n * sum(q["out"].n for q in qs) for _, x, qs in ch),
                        hbm_bytes=_distinct_bytes([x.grad for _, x, _ in ch] + [x.mask for _, x, _ in ch] +
                                                  [q["dC16"] for _, _, qs in ch for q in qs]) +
                        2.0 * sum(q["W"].data.numel() for _, _, qs in ch for q in qs))
            calls.append((L.load().mml_g16_tn, (descs, len(ch)), meta))
        return calls

    # ---- what the fp32 and the bf16-storage path share -----------------------------------------------------------
    def _relu_masks(self, plan):
        """Training plans: a ReLU output also leaves its sign bits (1 bit per element) for the dgrad that will apply
        relu' to its gradient -- 32x less to re-read than the activations themselves."""
        for q in self.p:
            out = q["out"]
            if plan.training and out.act == L.ACT_RELU and out.mask is None:
                out.mask = torch.zeros(plan.B, (out.n + 31) // 32, dtype=torch.int32, device=plan.device)

    def _live(self):
        """The problems whose output received a gradient."""
        return [q for q in self.p if q["out"].grad is not None]

    @staticmethod
    def _by_input(live):
        """[(x, the live problems that read x)] per distinct input value that takes a gradient, in order of appearance."""
        by_x = {}
        for q in live:
            if q["x"].needs_grad:
                by_x.setdefault(id(q["x"]), (q["x"], []))[1].append(q)
        return list(by_x.values())

    @staticmethod
    def _claim_wb(q):
        """Claim the weight and the bias gradient of problem q: (accumulate flag, bias gradient buffer or None)."""
        W, b = q["W"], q.get("b")
        acc = _claim(W)
        if b is not None and b.needs_grad and _claim(b) != acc:
            raise L.MMLError("weight and bias of one layer must be written in the same order")
        return acc, (b.grad if (b and b.needs_grad) else None)

    @staticmethod
    def _planes_all_or_none(wp):
        """Pre-cut weight planes [(planes, kexp)] for all problems / sources of a launch or for none: the kernels take
        the planes form per launch."""
        return wp if all(pl is not None for pl, _ in wp) else [(None, None)] * len(wp)

    def inputs(self):
        return [q["x"] for q in self.p] + [q["mul"] for q in self.p
                                           if q.get("mul") is not None and q.get("prod_bwd") != "ext"]

    def outputs(self):
        return [q["out"] for q in self.p] + [q["prod"] for q in self.p if q.get("mul") is not None]

    def _pad_calls(self, plan):
        """Reduction length not a multiple of 16: run the GEMM on the zero-padded operand pair (the value's own padded
        rows q["Ap"], a padded copy of the weight q["Wp"] refreshed every step by the copy returned here) instead of
        dropping to the register-staged kernel."""
        pads = []
        for q in self.p:
            kp = _kpad_of(q)
            if kp:
                q["Ap"] = _padded_view(q["x"].buf, kp)
                q["Wp"] = plan.zeros(q["W"].data.shape[0], kp)
                pads.append((q["W"].data, q["Wp"]))
        return [_copy2d_batch_call(plan, pads)] if pads else []

    def fwd_calls(self, plan):
        self._relu_masks(plan)
        if plan.bf16 and any(q["x"].is16 for q in self.p):
            self.use16 = True
            return self._fwd16(plan)
        pre = self._pad_calls(plan)
        # operand magnitudes: the input's (its producer's, or measured here), the weight's (start of the step), and the
        # output's is produced by this launch for the GEMMs that read it
        need = []
        for q in self.p:
            q["amax_a"] = plan.value_amax(q["x"], q.get("Ap", q["x"].buf), need)
            q["amax_w"] = plan.weight_amax(q["W"], q.get("Wp", q["W"].data), need)
            if q["out"].amax is None:
                q["out"].amax = plan.new_amax()
            if q.get("mul") is not None and q["prod"].amax is None:
                q["prod"].amax = plan.new_amax()
        if need:
            pre.append(plan.amax_call(need))
        wp = self._planes_all_or_none([plan.weight_planes(q, ops.PLANES_ROWS, padded="Wp" in q) for q in self.p])
        descs = ops.make_fwd_descs([dict(A=q.get("Ap", q["x"].buf), W=q.get("Wp", q["W"].data),
                                         bias=q["b"].data if q.get("b") else None,
                                         C=q["out"].buf, act=q["out"].act, w_kn=q.get("w_kn", 0),
                                         mask=q["out"].mask, amax_a=q["amax_a"], amax_w=q["amax_w"],
                                         amax_out=q["out"].amax, w_planes=pl, w_kexp=kx,
                                         mul=q["mul"].buf if q.get("mul") is not None else None,
                                         prod=q["prod"].buf if q.get("mul") is not None else None,
                                         amax_prod=q["prod"].amax if q.get("mul") is not None else None)
                                    for q, (pl, kx) in zip(self.p, wp)])
        plan.keep.append(descs)
        kn = self.p[0].get("w_kn", 0)
        meta = dict(kernel=_gemm_symbol(True, not kn, [q["out"].n for q in self.p], 0,
                                        kreds=[q.get("Ap", q["x"].buf).shape[1] for q in self.p],
                                        tensors=[q.get("Ap", q["x"].buf) for q in self.p] +
                                                [q.get("Wp", q["W"].data) for q in self.p],
                                        nrc_extents=[q["out"].n for q in self.p] if kn else []),
                    flops=sum(2.0 * plan.B * q["out"].n * q["x"].n for q in self.p),
                    hbm_bytes=_distinct_bytes([q["x"].buf for q in self.p] + [q["W"].data for q in self.p] +
                                              [q["out"].buf for q in self.p] + [q["out"].mask for q in self.p] +
                                              [q["prod"].buf for q in self.p if q.get("mul") is not None] +
                                              [q["mul"].buf for q in self.p if q.get("mul") is not None]))
        return pre + [(L.load().mml_gemm_grouped_fwd, (descs, len(self.p)), meta)]

    def bwd_calls(self, plan):
        live = self._live()
        if self.use16:
            return self._casts16(plan, live) + self._wgrad16_calls(plan, live) + self._dgrad16_calls(plan, live)
        # magnitudes of the incoming gradients (every writer of out.grad has been recorded by now): raised by the GEMM
        # that wrote them, else measured here, on the main chain, before the input-gradient and weight-gradient launches
        need = []
        for q in live:
            q["amax_dc"] = plan.grad_amax(q["out"], need)
            if q.get("amax_w") is None:
                q["amax_w"] = plan.weight_amax(q["W"], q.get("Wp", q["W"].data), need)
        calls = [plan.amax_call(need)] if need else []
        calls += self._wgrad_calls(plan, live)
        # input gradients: one dgrad problem per distinct input value
        waves = []  # chunk k of every input goes into launch k: chunks of ONE input must not run concurrently
        post = []   # sums of split input gradients, after the launches
        gate_wave = {}  # K7: id(factor value) -> last launch that writes its gradient
        for x, qs in self._by_input(live):
            if getattr(x, "gate", None) is not None:
                self._dgrad_gate(plan, x, qs, waves, gate_wave)
                continue
            plan.grad_of(x)
            if self._splits(plan, x, qs):
                post.append(self._dgrad_split(plan, x, qs, waves))
            else:
                self._dgrad_chunked(plan, x, qs, waves)
        return calls + self._dgrad_calls(plan, waves) + post

    def _wgrad_calls(self, plan, live):
        """Weight / bias gradients: the partial-product launch, its reduction, and the copies that un-pad the gradients of
        zero-padded weights -- all on the side list (only the optimizer reads them)."""
        lib = L.load()
        wg = []
        for q in live:
            W = q["W"]
            if not W.needs_grad:
                continue
            acc, dbias = self._claim_wb(q)
            if "Ap" in q and not acc:
                q["dWp"] = plan.empty(W.data.shape[0], q["Ap"].shape[1])
                wg.append(dict(dC=q["out"].grad, A=q["Ap"], dW=q["dWp"], dbias=dbias,
                               accumulate=0, w_kn=0, unpad=(q["dWp"], W.grad), amax_dc=q["amax_dc"],
                               amax_a=q.get("amax_a")))
                continue
            wg.append(dict(dC=q["out"].grad, A=q["x"].buf, dW=W.grad, dbias=dbias,
                           accumulate=acc, w_kn=q.get("w_kn", 0), amax_dc=q["amax_dc"], amax_a=q.get("amax_a")))
        if not wg:
            return []
        descs = ops.make_wgrad_descs(wg)
        nbytes = lib.mml_gemm_grouped_wgrad_workspace_bytes(descs, len(wg))
        # own workspace: all partial-product launches of the step run before the first reduction (see Plan)
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=plan.device)
        plan.keep += [descs, ws]
        meta = dict(kernel=_gemm_symbol(False, False, [q["dW"].shape[1] for q in wg], 2, kreds=[plan.B],
                                        tensors=[q["dC"] for q in wg] + [q["A"] for q in wg],
                                        nrc_extents=[d for q in wg for d in q["dW"].shape]),
                    flops=sum(2.0 * plan.B * q["dW"].numel() for q in wg), side=True, rank=0,
                    hbm_bytes=_distinct_bytes([q["dC"] for q in wg] + [q["A"] for q in wg] + [q["dW"] for q in wg]))
        calls = [(lib.mml_gemm_grouped_wgrad_phase, (descs, len(wg), ws.data_ptr(), ws.numel(), 1), meta),
                 (lib.mml_gemm_grouped_wgrad_phase, (descs, len(wg), ws.data_ptr(), ws.numel(), 2),
                  dict(kernel="slab_reduce", bytes=float(nbytes), side=True, rank=1))]
        unpad = [q["unpad"] for q in wg if "unpad" in q]  # padded weight gradients -> the parameters' [N, K]
        if unpad:
            c = _copy2d_batch_call(plan, unpad)
            call_meta(c)["side"] = True
            calls.append(c)
        return calls

    @staticmethod
    def _wave(waves, i):
        while len(waves) <= i:
            waves.append([])
        return waves[i]

    def _dgrad_gate(self, plan, x, qs, waves, gate_wave):
        """K7: x = h (.) g was written by the epilogue of the GEMM that produced g; its gradient is not stored, this
        problem writes the gradients of the two factors (gate mode)."""
        if len(qs) > L.MAX_SRC or len(x.consumers) != 1 or x.kpad:
            raise L.MMLError("a fused gate product must feed exactly one Linear group (<= MAX_SRC layers)")
        h, g = x.gate
        gd = dict(h=h.buf, g=g.buf)
        # h shared by several products and able to take its gradient in parts (MulBatchOp(fwd_fused)): this
        # problem writes a buffer of its own -- no accumulation, no order between the sharing problems
        parts = getattr(h, "grad_parts", None)
        # (at most seven: the summing launch takes eight terms per target -- parts + the plain gradient buffer a
        # further reader would add to)
        use_part = (parts is not None and h.act == L.ACT_NONE and len(parts) < 7 and
                    h.buf.stride(0) == h.n and plan.knobs.grad_parts)
        for key, v, nc in (("h", h, 1), ("g", g, 0)):
            if key == "h" and use_part:
                part = plan.empty(plan.B, h.n)
                parts.append(part)
                gd.update(dh=part, act_h=L.ACT_NONE, acc_h=0, amax_dh=None)
                continue
            gv = plan.grad_of(v)
            acc = _claim(v)
            fold = (not acc and v.act != L.ACT_NONE and not v.deriv_applied and len(v.consumers) == nc)
            if fold:
                v.deriv_applied = True
            gd.update({"d" + key: gv, "act_" + key: v.act if fold else L.ACT_NONE, "acc_" + key: acc,
                       "amax_d" + key: plan.grad_slot(v)})
        gp = self._planes_all_or_none([plan.weight_planes(q, ops.PLANES_COLS, qs) for q in qs])
        # products that share a factor (the gated input feeds every task's first product) write the SAME
        # gradient buffer, the first overwriting, the others adding: they must not run in one launch
        wi = max(-1 if use_part else gate_wave.get(id(h), -1), gate_wave.get(id(g), -1)) + 1
        gate_wave[id(g)] = wi
        if not use_part:
            gate_wave[id(h)] = wi
        self._wave(waves, wi).append(dict(
            dA=gd["dh"], gate=gd, Y=None, act=L.ACT_NONE, mask=None, accumulate=0,
            srcs=[(q["out"].grad, q["W"].data, q.get("w_kn", 0), q["amax_dc"], q["amax_w"]) +
                  ((pl, kx) if pl is not None else ()) for q, (pl, kx) in zip(qs, gp)]))

    @staticmethod
    def _grad_cols(plan, x, qs):
        """Columns of the input gradient somebody reads (Val.grad_cols), or 0 for all of them: a narrower launch over the
        same buffers."""
        return x.grad_cols if (0 < x.grad_cols < x.n and x.grad_cols % 16 == 0 and x.act == L.ACT_NONE and
                               all(isinstance(c, LinearGroupOp) for c in x.consumers) and
                               not any(q.get("w_kn", 0) for q in qs) and
                               plan.knobs.grad_cols) else 0

    @staticmethod
    def _splits(plan, x, qs):
        """Small batches: an input fed by many layers (dnn_input: every expert and gate) is ONE problem with a long
        reduction -- 128 tiles of 72 k-steps at B = 4 096 on AE-30, 41 us on a chip with 256 CUs.  Its sources are
        dealt to up to four problems of the same launch (partial sums into scratch, one add afterwards): 4x the
        tiles, a quarter of the steps.  Only without an activation derivative in the epilogue (input layers)."""
        return (plan.B <= 8192 and 2 <= len(qs) <= L.MAX_SRC and x.act == L.ACT_NONE and
                sum(q["out"].n for q in qs) >= 512 and plan.knobs.split_dgrad)

    def _dgrad_split(self, plan, x, qs, waves):
        """The split problem (_splits): up to four problems of the first launch; returns the call that sums the parts."""
        gc = self._grad_cols(plan, x, qs)
        cut = (lambda t: t[:, :gc]) if gc else (lambda t: t)
        nparts = min(4, len(qs))
        parts = [[] for _ in range(nparts)]
        for q in sorted(qs, key=lambda q_: -q_["out"].n):  # longest first into the lightest part
            min(parts, key=lambda p_: sum(r["out"].n for r in p_)).append(q)
        acc = _claim(x)
        padded = x.kpad and all("Wp" in q for q in qs)
        g0 = cut(_padded_view(x.grad, x.kpad) if padded else x.grad)
        pitch = x.grad.stride(0)
        targets = [g0]
        for _ in parts[1:]:
            t_ = plan.zeros(plan.B, pitch)
            targets.append(t_.as_strided(g0.shape, (pitch, 1)))
        for part, dst in zip(parts, targets):
            self._wave(waves, 0).append(dict(
                dA=dst, Y=None, act=L.ACT_NONE, mask=None, accumulate=acc if dst is g0 else 0,
                srcs=[(q["out"].grad, cut(q["Wp"] if padded else q["W"].data), q.get("w_kn", 0),
                       q["amax_dc"], q["amax_w"]) for q in part]))
        return plan.bound(bind.ew_add_n([x.grad] + targets[1:], x.grad, n=plan.B * pitch),
                          kernel="ew_add_n_kernel", bytes=4.0 * plan.B * pitch * (len(targets) + 1))

    def _dgrad_chunked(self, plan, x, qs, waves):
        """The plain problem: the layers that read x in chunks of MAX_SRC sources, chunk k in launch k."""
        chunks = [qs[i:i + L.MAX_SRC] for i in range(0, len(qs), L.MAX_SRC)]
        fuse = len(chunks) == 1 and len(x.consumers) == 1 and x.act != L.ACT_NONE
        gc = self._grad_cols(plan, x, qs)
        cut = (lambda t: t[:, :gc]) if gc else (lambda t: t)
        for ci, ch in enumerate(chunks):
            acc = _claim(x)
            padded = x.kpad and all("Wp" in q for q in ch)  # every source reads the zero-padded weight copy
            # this launch raises the magnitude slot of x.grad with what it stores (after derivative / accumulation)
            out_slot = plan.grad_slot(x)
            # the weights that feed this input gradient, cut as one group (common exponent)
            gp = self._planes_all_or_none([plan.weight_planes(q, ops.PLANES_COLS, ch, padded=bool(padded)) for q in ch])
            # a launch that raises the slot and stores exactly x.grad's [B, n] region: if the output-stationary kernel
            # serves it (_dgrad_calls asks the library), the slot holds the exact maximum of what was stored
            exact = out_slot is not None and not x.kpad and not gc
            self._wave(waves, ci).append(dict(
                dA=cut(_padded_view(x.grad, x.kpad) if padded else x.grad),
                Y=x.buf if fuse else None, act=x.act if fuse else L.ACT_NONE,
                mask=x.mask if (fuse and x.act == L.ACT_RELU) else None,
                accumulate=acc, amax_out=out_slot, exact_amax_of=x if exact else None,
                srcs=[(q["out"].grad, cut(q["Wp"] if padded else q["W"].data), q.get("w_kn", 0),
                       q["amax_dc"], q["amax_w"]) + ((pl, kx) if pl is not None else ())
                      for q, (pl, kx) in zip(ch, gp)]))
        if fuse:
            x.deriv_applied = True

    @staticmethod
    def _dgrad_calls(plan, waves):
        """One mml_gemm_grouped_dgrad call per wave of input-gradient problems."""
        lib = L.load()
        calls = []
        for dg in waves:
            descs = ops.make_dgrad_descs(dg)
            plan.keep.append(descs)
            # csrc/gemm_os.hip (one problem per launch) raises the slot with the exact maximum of what it stored:
            # GatherOp's deterministic scatter may take its fixed-point unit from it
            # (tests/test_scatter_det_fused_gpu.py).  Whether that kernel runs is the library's decision.
            x = dg[0].get("exact_amax_of") if len(dg) == 1 else None
            if x is not None and lib.mml_gemm_os_serves(descs, len(dg)):
                x.gamax_exact = True
            kn = dg[0]["srcs"][0][2]
            meta = dict(kernel=_gemm_symbol(True, bool(kn), [q["dA"].shape[1] for q in dg], 1,
                                            kreds=[sr[0].shape[1] for q in dg for sr in q["srcs"]],
                                            tensors=[t_ for q in dg for sr in q["srcs"] for t_ in sr[:2]],
                                            nrc_extents=[] if kn else [q["dA"].shape[1] for q in dg]),
                        flops=sum(2.0 * plan.B * q["dA"].shape[1] * sum(sr[0].shape[1] for sr in q["srcs"])
                                  for q in dg),
                        hbm_bytes=_distinct_bytes([q["dA"] for q in dg] + [q.get("mask") for q in dg] +
                                                  [t_ for q in dg for sr in q["srcs"] for t_ in sr[:2]]))
            calls.append((lib.mml_gemm_grouped_dgrad, (descs, len(dg)), meta))
        return calls


class GateGroupOp(Op):
    """K4: gates (skinny linear + softmax) mixing a shared list of expert outputs.
    gates: dicts with G (Val), Wg (PVal), mix (Val), expert (indices into `experts`)."""

    def __init__(self, experts, gates, H):
        self.experts, self.gates, self.H = experts, gates, H

    def writes_grad16(self, plan, v):
        # (the fast backward writes dE / dG as bf16: mml_gate_group.out_bf16; whether it serves the group is the library's rule)
        shape = gate_rows_shape(self.H, max(g["G"].n for g in self.gates), len(self.experts), len(self.gates),
                                any(e.is16 for e in self.experts))
        return bool(shape & L.GATE_SHAPE_FAST_BWD)

    def inputs(self):
        return list(self.experts) + [g["G"] for g in self.gates]

    def outputs(self):
        return [g["mix"] for g in self.gates]

    def fwd_calls(self, plan):
        for g in self.gates:
            g["P"] = plan.empty(plan.B, len(g["expert"]))
        grp = ops.make_gate_group([e.buf for e in self.experts],
                                  [dict(G=g["G"].buf, Wg=g["Wg"].data, P=g["P"], mix=g["mix"].buf, expert=g["expert"])
                                   for g in self.gates], plan.B, self.H)
        slot = plan.new_amax()  # ONE magnitude slot for all mixtures (an upper bound for each of them)
        if slot is not None:
            grp.amax_mix = slot.data_ptr()
            for g in self.gates:
                g["mix"].amax = slot
        plan.keep.append(grp)
        byts = 4.0 * plan.B * (len(self.experts) * self.H + sum(g["G"].n + len(g["expert"]) + self.H for g in self.gates))
        return [(L.load().mml_gate_mix_fwd, (C.byref(grp),), dict(kernel="gate_fwd_kernel", bytes=byts))]

    def bwd_calls(self, plan):
        lib = L.load()
        if all(g["mix"].grad is None for g in self.gates):
            return []
        for e in self.experts:
            if e.needs_grad and (len(e.consumers) != 1 or e.written):
                raise NotImplementedError("an expert output feeding something besides one gate group")
        e_relu = all(e.act == L.ACT_RELU for e in self.experts)
        if not e_relu and any(e.act != L.ACT_NONE for e in self.experts):
            raise NotImplementedError("gate group over experts with mixed activations")
        gl = []
        for g in self.gates:
            G, active = g["G"], g["mix"].grad is not None
            q = dict(G=G.buf, Wg=g["Wg"].data, P=g["P"], expert=g["expert"], active=int(active))
            if active:
                if G.needs_grad and (len(G.consumers) != 1 or G.written):
                    raise NotImplementedError("a gate input feeding something besides its gate")
                if _claim(g["Wg"]):
                    raise NotImplementedError("a gate weight shared between gates")
                fuse = G.act == L.ACT_RELU
                if G.act not in (L.ACT_RELU, L.ACT_NONE):
                    raise NotImplementedError("gate input activation")
                q.update(dmix=g["mix"].grad, dG=plan.grad_of(G), dWg=g["Wg"].grad, g_relu=int(fuse))
                _claim(G)
                G.deriv_applied = True
            gl.append(q)
        dE = []
        for e in self.experts:
            dE.append(plan.grad_of(e))
            _claim(e)
            e.deriv_applied = True
        grp = ops.make_gate_group([e.buf for e in self.experts], gl, plan.B, self.H, d_experts=dE, e_relu=e_relu)
        # magnitudes of what the kernel stores: one slot for every expert gradient, one for every gate-input gradient
        # (this op is the only writer of each of them: checked above)
        s_de = plan.shared_grad_slot(self.experts)
        s_dg = plan.shared_grad_slot([g["G"] for g in self.gates if g["mix"].grad is not None])
        if s_de is not None:
            grp.amax_dE, grp.amax_dG = s_de.data_ptr(), s_dg.data_ptr()
        nws = int(lib.mml_gate_mix_bwd_workspace_bytes(C.byref(grp)))
        # (deferred reduction: the partial sums must survive until the side list runs -- a buffer of this op's own, not the
        # shared scratch every other call overwrites)
        ws = (torch.empty(max(nws, 256), dtype=torch.uint8, device=plan.device) if _defer_reduce()
              else ops.workspace(nws, plan.device))
        plan.keep += [grp, ws]
        act = [g for g in self.gates if g["mix"].grad is not None]
        byts = 4.0 * plan.B * (2 * len(self.experts) * self.H + sum(2 * g["G"].n + len(g["expert"]) + self.H for g in act))
        if _defer_reduce():
            # only the optimizer reads dWg: the reduction of the per-workgroup partial sums leaves the backward chain and
            # runs beside the weight-gradient GEMMs (the workspace is this op's own)
            return [(lib.mml_gate_mix_bwd_phase, (C.byref(grp), ws.data_ptr(), ws.numel(), 1),
                     dict(kernel="gate_bwd_kernel", bytes=byts)),
                    (lib.mml_gate_mix_bwd_phase, (C.byref(grp), ws.data_ptr(), ws.numel(), 2),
                     dict(kernel="slab_reduce", bytes=float(ws.numel()), side=True, rank=1))]
        return [(lib.mml_gate_mix_bwd, (C.byref(grp), ws.data_ptr(), ws.numel()),
                 dict(kernel="gate_bwd_kernel", bytes=byts))]


_DEFER = None  # inside deferred_reductions(on): `on`


@contextlib.contextmanager
def deferred_reductions(on):
    """While a plan is recorded inside this block, GateGroupOp / HeadOp defer their reductions iff `on`
    (trainer.TrainStep: a step that runs as ONE list); MMLREC_DEFER_REDUCE still overrides (_defer_reduce)."""
    global _DEFER
    prev, _DEFER = _DEFER, on
    try:
        yield
    finally:
        _DEFER = prev


def _defer_reduce():
    """MMLREC_DEFER_REDUCE=1: the reductions of the gate / head kernels' partial sums (only the optimizer reads their
    results) leave the backward chain and run beside the weight-gradient GEMMs (mml_gate_mix_bwd_phase,
    mml_head_bce_fwd_bwd_phase).  Off by default: two launches fewer on the chain (-18 us in a serial trace of the AE-30
    step), but the two-stream step measured 1.702 against 1.666 ms with it (three interleaved pairs, round 4) -- the step
    is bound by what its kernels take from HBM and the CUs together, not by the length of the chain."""
    e = os.environ.get("MMLREC_DEFER_REDUCE")
    if e is not None:
        return e == "1"
    # Round 5, ONE stream: deferred, and passes.merge_row_reduces turns the deferred reductions of a step into ONE launch
    # (mml_rows_reduce_batch): MMoE one launch fewer per step, a PLE of two levels two.
    return bool(_DEFER)


class HeadOp(Op):
    """K5: prediction heads (+ the summed loss and its backward when training).
    heads: dicts with Hin (Val), w (PVal with H elements), bias (PVal [1]), bias2 (PVal [1] or None), kind (L.head_kind(out,
    loss), default 0 = sigmoid + BCE; BaseModel._finish_record fills it from task_types and the compiled losses); a gated head (round 6,
    PepNet's last PPNet layer, reference model/pepnet.py:72-78) also carries gate (Val: the input of the head is
    Hin (.) gate, formed inside the kernel; this op must be the only consumer of both values)."""

    def __init__(self, heads, mask_cols=None):
        self.heads = heads
        self.mask_cols = mask_cols

    def writes_grad16(self, plan, v):
        # (the fast head kernel writes dH as bf16: mml_head_group.dh_bf16 -- all heads or none)
        return (type(self) is HeadOp and all(_fast_row_width_ok(h["Hin"].n) for h in self.heads) and
                all(h["Hin"].producer16 and h["Hin"].n % 8 == 0 and len(h["Hin"].consumers) == 1 for h in self.heads))

    def inputs(self):
        return [h["Hin"] for h in self.heads] + [h["gate"] for h in self.heads if h.get("gate") is not None]

    def _group(self, plan, train, use_dprob, claim):
        T = len(self.heads)
        if plan.prob is None:
            plan.prob = plan.empty(plan.B, T)
        prob_buf, dprob_buf = self._prob_buffers(plan, use_dprob)
        hl, post = [], []
        for t, h in enumerate(self.heads):
            Hin = h["Hin"]
            q = dict(Hin=Hin.buf, w=h["w"].data, bias=h["bias"].data,
                     bias2=h["bias2"].data if h.get("bias2") is not None else None,
                     mask_col=(self.mask_cols[t] if (self.mask_cols and plan.mask is not None) else -1),
                     kind=int(h.get("kind", 0)))  # (include/mmlrec.h K5: output form and loss of the head)
            G = h.get("gate")
            if G is not None:
                if G.n != Hin.n or not _fast_row_width_ok(Hin.n) or Hin.is16 or G.is16:
                    raise L.MMLError("gated head: gate and input of one width the fast row kernel serves, fp32")
                q.update(gate=G.buf, gate_act=G.act)
            if train:
                sole = len(Hin.consumers) == 1
                if G is not None:
                    if not sole or len(G.consumers) != 1 or G.act not in (L.ACT_NONE, L.ACT_SIGMOID, L.ACT_SIGMOID2):
                        raise L.MMLError("gated head: the head must be the only consumer of its input and of its gate")
                    q["dgate"] = plan.grad_of(G)
                    if claim:
                        if _claim(G):
                            raise L.MMLError("gated head: the gate's gradient has another writer")
                        G.deriv_applied = True   # (the kernel multiplies act'(gate) in)
                        # ONE slot for all gates' gradients
                        self._amax_dG = plan.shared_grad_slot([G], getattr(self, "_amax_dG", None))
                if sole:
                    q["dH"] = plan.grad_of(Hin)
                    q["h_relu"] = int(Hin.act == L.ACT_RELU)
                    if Hin.act not in (L.ACT_RELU, L.ACT_NONE):
                        raise NotImplementedError("head input activation")
                    if claim:
                        _claim(Hin)
                        Hin.deriv_applied = True
                        if Hin.written == 1:  # the kernel raises ONE slot for all dH
                            self._amax_dH = plan.shared_grad_slot([Hin], getattr(self, "_amax_dH", None))
                else:
                    tmp = h.setdefault("_dH_tmp", plan.empty(plan.B, Hin.n))
                    q["dH"], q["h_relu"] = tmp, 0
                    plan.grad_of(Hin)
                    acc = _claim(Hin) if claim else h["_acc"]
                    h["_acc"] = acc
                    post.append(plan.bound(bind.copy2d(tmp, Hin.grad, acc)))
                if claim:
                    h["_acc_w"] = _claim(h["w"])
                    h["_acc_b"] = _claim(h["bias"])
                if h["_acc_b"]:  # a bias shared by several heads (reference model/esmm.py:55-56: one PredictionLayer)
                    tmpb = h.setdefault("_db_tmp", plan.empty(1))
                    q["dbias"] = tmpb
                    post.append(plan.bound(bind.copy_flat(tmpb, h["bias"].grad, 1)))
                else:
                    q["dbias"] = h["bias"].grad
                if h["_acc_w"]:
                    # a weight shared by several heads (reference model/mlp.py:28): this head's gradient goes to a
                    # scratch row that is added to the parameter's gradient after the launch
                    tmpw = h.setdefault("_dw_tmp", plan.empty(h["w"].data.numel()))
                    q["dw"] = tmpw
                    post.append(plan.bound(bind.copy_flat(tmpw, h["w"].grad, 1)))
                else:
                    q["dw"] = h["w"].grad
                b2 = h.get("bias2")
                if b2 is not None and b2.needs_grad:
                    acc = _claim(b2) if claim else h["_acc_b2"]
                    h["_acc_b2"] = acc
                    post.append(plan.bound(bind.copy_flat(h["bias"].grad, b2.grad, acc, n=1)))
            hl.append(q)
        grp = ops.make_head_group(hl, prob_buf, y=plan.y if (train and not use_dprob) else None, mask=plan.mask,
                                  loss=plan.loss if (train and not use_dprob) else None,
                                  dprob=dprob_buf if use_dprob else None)
        if train and getattr(self, "_amax_dH", None) is not None:
            grp.amax_dH = self._amax_dH.data_ptr()
        if train and getattr(self, "_amax_dG", None) is not None:
            grp.amax_dG = self._amax_dG.data_ptr()
        plan.keep.append(grp)
        return grp, post

    def _prob_buffers(self, plan, use_dprob):
        """(where the heads write their probabilities, where they read dL/dprob from)."""
        return plan.prob, plan.dprob

    def infer_calls(self, plan):
        grp, _ = self._group(plan, False, False, False)
        return [(L.load().mml_head_fwd, (C.byref(grp),),
                 dict(kernel="head_kernel", bytes=4.0 * plan.B * sum(h["Hin"].n + 1 for h in self.heads)))]

    def train_calls(self, plan, use_dprob, claim=True):
        lib = L.load()
        if use_dprob and plan.dprob is None:
            plan.dprob = plan.empty(plan.B, len(self.heads))
        grp, post = self._group(plan, True, use_dprob, claim)
        defer = not use_dprob and not post and _defer_reduce()
        nws = int(lib.mml_head_workspace_bytes(C.byref(grp)))
        ws = (torch.empty(max(nws, 256), dtype=torch.uint8, device=plan.device) if defer  # (its own: see GateGroupOp)
              else ops.workspace(nws, plan.device))
        plan.keep.append(ws)
        byts = 4.0 * plan.B * sum((4 if h.get("gate") is not None else 2) * h["Hin"].n + 2 for h in self.heads)
        if defer:
            # (dw / dbias / loss are read by the optimizer and the host only: their reduction runs beside the
            # weight-gradient GEMMs; Plan.finish moves the call tagged `side` out of the head's list)
            return [(lib.mml_head_bce_fwd_bwd_phase, (C.byref(grp), ws.data_ptr(), ws.numel(), 1),
                     dict(kernel="head_kernel", bytes=byts)),
                    (lib.mml_head_bce_fwd_bwd_phase, (C.byref(grp), ws.data_ptr(), ws.numel(), 2),
                     dict(kernel="slab_reduce", bytes=float(ws.numel()), side=True, rank=1, ready=0))]
        return [(lib.mml_head_bce_fwd_bwd, (C.byref(grp), ws.data_ptr(), ws.numel()),
                 dict(kernel="head_kernel", bytes=byts))] + post


class EsmmHeadOp(HeadOp):
    """ESMM (reference model/esmm.py:46-62): two sigmoid heads (ctr, cvr) whose product is the second output.
    The heads run on a raw probability buffer; mml_esmm_combine turns it into [ctr, ctr*cvr], evaluates the summed BCE
    and hands dLoss/d(ctr, cvr) back to the head kernel's dprob path."""
    N_OUT = 2
    KERNEL = "esmm_combine_kernel"

    def _group(self, plan, *a):
        if plan.prob is None:
            plan.prob = plan.empty(plan.B, self.N_OUT)
        return super()._group(plan, *a)

    def _prob_buffers(self, plan, use_dprob):
        if getattr(self, "_raw", None) is None or self._raw.shape[0] != plan.B:
            self._raw = plan.empty(plan.B, 2)
            self._draw = plan.empty(plan.B, 2)
        return self._raw, self._draw

    def _bind(self, *a):
        return bind.esmm_combine(*a)

    def _combine(self, plan, y, dout, draw, loss):
        return plan.bound(self._bind(self._raw, y, dout, plan.prob, draw, loss, plan.B),
                          kernel=self.KERNEL, bytes=4.0 * plan.B * 8)

    def infer_calls(self, plan):
        calls = super().infer_calls(plan)
        return calls + [self._combine(plan, None, None, None, None)]

    def train_calls(self, plan, use_dprob, claim=True):
        lib = L.load()
        if use_dprob:  # autograd hands dL/d(outputs); the raw probabilities are those of the forward pass
            if plan.dprob is None:
                plan.dprob = plan.empty(plan.B, self.N_OUT)
            pre = [self._combine(plan, None, plan.dprob, self._prob_buffers(plan, True)[1], None)]
        else:
            fwd, _ = self._group(plan, False, False, False)
            if plan.y.stride(0) != 2:
                raise L.MMLError("ESMM / ESCM expect a contiguous [B, 2] label buffer")
            pre = [(lib.mml_head_fwd, (C.byref(fwd),), dict(kernel="head_kernel")),
                   self._combine(plan, plan.y, None, self._draw, plan.loss)]
        grp, post = self._group(plan, True, True, claim)
        ws = ops.workspace(lib.mml_head_workspace_bytes(C.byref(grp)), plan.device)
        plan.keep.append(ws)
        byts = 4.0 * plan.B * sum(2 * h["Hin"].n + 2 for h in self.heads)
        return pre + [(lib.mml_head_bce_fwd_bwd, (C.byref(grp), ws.data_ptr(), ws.numel()),
                       dict(kernel="head_kernel", bytes=byts))] + post


class EscmHeadOp(EsmmHeadOp):
    """ESCM (reference model/escm.py:74-112): outputs [ctr, cvr, ctr*cvr]; the training loss is the reference's
    special branch (model/basemodel.py:284-292: BCE(ctr) + 0.1 * counterfactual-IPW(cvr) + BCE(ctcvr)), evaluated with
    its gradient by mml_escm_combine."""
    N_OUT = 3
    KERNEL = "escm_combine_kernel"

    def __init__(self, heads, cf_w, global_w, mask_cols=None):
        super().__init__(heads, mask_cols)
        self.cf_w, self.global_w = float(cf_w), float(global_w)

    def _bind(self, *a):
        return bind.escm_combine(*a, self.cf_w, self.global_w)


class BNOp(Op):
    """BatchNorm1d between a layer's Linear and its activation (reference model/utils.py:153-157): z -> y = act(bn(z)).
    Batch statistics (and the in-place running-statistics update) when the module is in training mode, running
    statistics otherwise -- `plan.bn_training`, NOT plan.training: a no_grad forward of a model in train() mode still
    normalises with the batch and moves the running statistics, exactly like torch."""
    EPS, MOMENTUM = 1e-5, 0.1

    def __init__(self, z, y, gamma, beta, module):
        self.z, self.y, self.gamma, self.beta, self.m = z, y, gamma, beta, module

    def inputs(self):
        return [self.z]

    def outputs(self):
        return [self.y]

    def fwd_calls(self, plan):
        n = self.z.n
        self.mean, self.rstd = plan.empty(n), plan.empty(n)
        m = self.m
        return [plan.bound(bind.bn_fwd(self.z.buf, self.gamma.data, self.beta.data, m.running_mean, m.running_var,
                                       m.num_batches_tracked, self.mean, self.rstd, self.y.buf, self.y.act,
                                       getattr(plan, "bn_training", plan.training), self.EPS, self.MOMENTUM,
                                       plan.workspace(L.load().mml_bn_workspace_bytes(plan.B, n))),
                           kernel="bn_fwd", bytes=4.0 * plan.B * n * 3)]

    def bwd_calls(self, plan):
        if self.y.grad is None:
            return []
        if not getattr(plan, "bn_training", plan.training):
            raise L.MMLError("backward through BatchNorm in eval mode is not supported")
        plan.grad_of(self.z)
        _claim(self.z)
        acc = _claim(self.gamma)
        if _claim(self.beta) != acc:
            raise L.MMLError("BatchNorm weight and bias must be written in the same order")
        n = self.z.n
        return [plan.bound(bind.bn_bwd(self.y.grad, self.z.buf, self.gamma.data, self.mean, self.rstd, self.z.grad,
                                       self.gamma.grad, self.beta.grad, acc,
                                       plan.workspace(L.load().mml_bn_workspace_bytes(plan.B, n))),
                           kernel="bn_bwd", bytes=4.0 * plan.B * n * 5)]


class DropoutOp(Op):
    """nn.Dropout after a DNN layer's activation (reference model/utils.py:121, :159): x -> y = x * keep / (1 - p) while
    the module is in training mode (`plan.dropout_on`, recorded like BatchNorm's mode; in eval mode the model does not
    add the op).  The mask is regenerated, not stored (mml_dropout): the backward is the same call on dL/dy with the
    step counter the forward read -- the optimizer's device counter, bumped at the start of a fused step."""

    def __init__(self, x, y, p, seed, site):
        self.x, self.y, self.p, self.seed, self.site = x, y, float(p), seed, site  # (bind.dropout cuts seed / site to size)

    def inputs(self):
        return [self.x]

    def outputs(self):
        return [self.y]

    def _call(self, plan, src, dst, acc):
        return plan.bound(bind.dropout(src, dst, self.p, self.seed, self.site, plan.step_dev, 0, acc, plan.row0, rows=plan.B),
                          kernel="dropout_kernel", bytes=4.0 * plan.B * self.x.n * (3 if acc else 2))

    def fwd_calls(self, plan):
        return [self._call(plan, self.x.buf, self.y.buf, 0)]

    def bwd_calls(self, plan):
        if self.y.grad is None or not self.x.needs_grad:
            return []
        g = plan.grad_of(self.x)
        return [self._call(plan, self.y.grad, g, _claim(self.x))]


class PReluBatchOp(Op):
    """nn.PReLU() of one layer depth of sibling stacks (reference model/utils.py:25-26, :156-157; STAR model/star.py:47-49):
    y_j = z_j > 0 ? z_j : a_j * z_j for every stack in ONE launch each way (mml_prelu_batch_fwd / _bwd).
    items: (z Val, y Val, alpha PVal); both values carry ACT_NONE -- downstream, y is the output of a `linear` layer.  The
    backward reads z (kept: for a slope <= 0 the sign of y does not give the sign of z), writes dL/dz once and claims the
    slope's gradient like BatchNorm's gamma; items that share a slope (STAR: one per layer, every domain) are summed by the
    launch.  Where the plan has a magnitude pool the launches raise the slots of y and of dL/dz themselves."""

    def __init__(self, items):
        self.items = list(items)
        for z, y, _ in self.items:
            if z.act != L.ACT_NONE or y.act != L.ACT_NONE or z.is16 or y.is16 or z.n != y.n:
                raise L.MMLError("PReluBatchOp: fp32 values of one width without an activation of their own")

    def inputs(self):
        return [z for z, _, _ in self.items]

    def outputs(self):
        return [y for _, y, _ in self.items]

    def fwd_calls(self, plan):
        rows = []
        for z, y, a in self.items:
            if y.amax is None:
                y.amax = plan.new_amax()
            rows.append(dict(z=z.buf, y=y.buf, alpha=a.data, amax=y.amax))
        calls = []
        for ch in ops.prelu_chunks(rows):
            arr = ops.make_prelu_descs(ch)
            plan.keep.append(arr)
            calls.append((L.load().mml_prelu_batch_fwd, (arr, len(ch)),
                          dict(kernel="prelu_fwd_kernel", bytes=8.0 * sum(r["z"].numel() for r in ch))))
        return calls

    def bwd_calls(self, plan):
        rows, acc_da = [], {}
        for z, y, a in self.items:
            if y.grad is None or not (z.needs_grad or a.needs_grad):
                continue
            if y.grad.dtype != torch.float32:
                raise L.MMLError(f"PReLU output {y.name!r}: its gradient must be fp32")
            g = plan.grad_of(z)
            acc = _claim(z)
            if id(a) not in acc_da:  # (later items of the slope: the launch sums them behind the first)
                acc_da[id(a)] = _claim(a)
            # (amax: magnitude of the gradient as stored, tracked like a dgrad GEMM's amax_out)
            rows.append(dict(dy=y.grad, z=z.buf, dz=g, alpha=a.data, dalpha=a.grad, acc_dz=acc,
                             acc_dalpha=acc_da[id(a)], amax=plan.grad_slot(z)))
        calls, seen = [], set()
        for ch in ops.prelu_chunks(rows):
            arr = ops.make_prelu_bwd_descs(ch, seen)
            seen.update(d.dalpha for d in arr)
            ws = plan.workspace(L.load().mml_prelu_workspace_bytes(len(ch)))
            plan.keep.append(arr)
            calls.append((L.load().mml_prelu_batch_bwd, (arr, len(ch), ws.data_ptr(), ws.numel()),
                          dict(kernel="prelu_bwd_kernel", bytes=sum((16.0 if r["acc_dz"] else 12.0) * r["z"].numel()
                                                                    for r in ch))))
        return calls


def dropout_site(name):
    """The `site` word of a dropout layer's mask stream: CRC-32 of the layer's name (prefix.layer), so that the engine
    and the CPU restatement (oracle/mmlrec_oracle.py) agree without sharing a counter."""
    import zlib
    return zlib.crc32(name.encode()) & 0xffffffff


class DomainBNOp(Op):
    """DomainBatchNorm of STAR (reference model/utils.py:553-636, applied after the first star layer's activation when
    forward() is given a domain mask, model/star.py:50-51): x (a post-activation value) -> y.  gamma / beta are the
    reference's unregistered constants (1, 0).  Training mode = whole-batch statistics (mml_bn_fwd) plus the per-domain
    population-statistics update; eval mode = per-domain normalisation with the population statistics.

    Training mode assumes ONE-HOT mask rows (what get_mask, model/utils.py:639-645, produces): the reference's
    sum_d mask[b, d] * BN_batch(x[b]) then equals BN_batch(x[b]).  A row whose mask is all zero (or holds several
    ones) would need the factor sum_d mask[b, d]; such masks are outside the contract of this op."""
    EPS, DECAY = 1e-5, 0.99

    def __init__(self, x, y, module, mask):
        self.x, self.y, self.m, self.mask = x, y, module, mask

    def inputs(self):
        return [self.x]

    def outputs(self):
        return [self.y]

    def fwd_calls(self, plan):
        n, D = self.x.n, self.mask.shape[1]
        pm, pv = self.m.population(plan.device)
        if pm.shape != (D, n):
            raise L.MMLError(f"DomainBatchNorm holds {tuple(pm.shape)} statistics, the mask has {D} domains")
        x, y = self.x.buf, self.y.buf
        if not getattr(plan, "bn_training", plan.training):
            return [plan.bound(bind.domain_bn_eval(x, self.mask, pm, pv, y, self.EPS), kernel="domain_bn_eval_kernel")]
        self.ones, self.zeros = torch.ones(n, device=plan.device), torch.zeros(n, device=plan.device)
        self.mean, self.rstd = plan.empty(n), plan.empty(n)
        self.scratch = [plan.zeros(n), plan.zeros(n), plan.zeros(1, dtype=torch.int64)]  # F.batch_norm's discarded running stats
        plan.keep += [self.ones, self.zeros]
        return [plan.bound(bind.domain_bn_update(x, self.mask, pm, pv, self.DECAY), kernel="domain_bn_update_kernel"),
                plan.bound(bind.bn_fwd(x, self.ones, self.zeros, *self.scratch, self.mean, self.rstd, y, L.ACT_NONE, 1,
                                       self.EPS, 0.1, plan.workspace(L.load().mml_bn_workspace_bytes(plan.B, n))),
                           kernel="bn_fwd")]

    def bwd_calls(self, plan):
        if self.y.grad is None:
            return []
        if not getattr(plan, "bn_training", plan.training):
            raise L.MMLError("backward through DomainBatchNorm in eval mode is not supported")
        plan.grad_of(self.x)
        if _claim(self.x):
            raise NotImplementedError("DomainBatchNorm input with another consumer")
        n = self.x.n
        dscr = plan.empty(2 * n)  # (dgamma, dbeta of the constant gamma / beta: discarded)
        return [plan.bound(bind.bn_bwd(self.y.grad, self.x.buf, self.ones, self.mean, self.rstd, self.x.grad, dscr, dscr[n:],
                                       0, plan.workspace(L.load().mml_bn_workspace_bytes(plan.B, n))), kernel="bn_bwd")]


class ApgFeatOp(Op):
    """z = [o1 (x) s | o1 | s | 0] (csrc/apg.hip): the feature row that turns APG's per-sample generated [k,k] weight
    into one GEMM (reference model/apg.py:77-80, :100-104).  s is the detached scene embedding (a column slice of
    dnn_input): no gradient flows into it."""

    def __init__(self, o1, s, z, k, E):
        self.o1, self.s, self.z, self.k, self.E = o1, s, z, k, E

    def inputs(self):
        return [self.o1]

    def outputs(self):
        return [self.z]

    def fwd_calls(self, plan):
        return [plan.bound(bind.apg_features_fwd(self.o1.buf, self.s, self.z.buf, self.k, self.E),
                           kernel="apg_features_fwd_kernel", bytes=4.0 * plan.B * (self.z.n + self.k + self.E))]

    def bwd_calls(self, plan):
        if self.z.grad is None or not self.o1.needs_grad:
            return []
        if self.o1.act != L.ACT_NONE:
            raise NotImplementedError("ApgFeatOp input must be a plain linear output")
        do1 = plan.grad_of(self.o1)
        acc = _claim(self.o1)
        return [plan.bound(bind.apg_features_bwd(self.z.grad, self.s, do1, self.k, self.E, acc),
                           kernel="apg_features_bwd_kernel", bytes=4.0 * plan.B * (self.z.n + self.k + self.E))]


class ApgWeightsOp(Op):
    """Derived [Kf, k] weight of an APG layer's middle GEMM, re-laid-out from the generator Linear(E -> k*k) (weight
    Wkk, bias bkk) and the weight of the generator Linear(E -> k) of the per-sample bias (csrc/apg.hip); backward
    unpacks its gradient into theirs."""

    def __init__(self, Wkk, bkk, Wb, Wcat, k, E):
        self.Wkk, self.bkk, self.Wb, self.Wcat, self.k, self.E = Wkk, bkk, Wb, Wcat, k, E

    def fwd_calls(self, plan):
        return [plan.bound(bind.apg_weights(self.Wkk.data, self.bkk.data, self.Wb.data, self.Wcat.data, self.k, self.E, 0),
                           kernel="apg_weights_kernel")]

    def bwd_calls(self, plan):
        if not self.Wcat.written:
            return []
        acc = (_claim(self.Wkk), _claim(self.bkk), _claim(self.Wb))
        return [plan.bound(bind.apg_weights(self.Wkk.grad, self.bkk.grad, self.Wb.grad, self.Wcat.grad, self.k, self.E, 1,
                                            acc), kernel="apg_weights_kernel", side=True)]


class Attn2Op(Op):
    """Two-token attention of AITM (model/aitm.py:84-93): tokens = [(V0, K0, Q0), (V1, K1, Q1)] of [B, H] values -> out."""

    def __init__(self, tokens, out, sqrt_h):
        self.tokens, self.out, self.sqrt_h = tokens, out, float(sqrt_h)

    def inputs(self):
        return [v for tok in self.tokens for v in tok]

    def outputs(self):
        return [self.out]

    def _desc(self, plan, grads=None):
        d = ops.make_attn2_desc([[v.buf for v in tok] for tok in self.tokens], self.out.buf, self.A, plan.B, self.out.n,
                                self.sqrt_h, grads)
        plan.keep.append(d)
        return d

    def fwd_calls(self, plan):
        self.A = plan.empty(plan.B, 2)
        d = self._desc(plan)
        return [(L.load().mml_attn2_fwd, (C.byref(d),), dict(kernel="attn2_fwd_kernel", bytes=4.0 * plan.B * 7 * self.out.n))]

    def bwd_calls(self, plan):
        if self.out.grad is None:
            return []
        for v in self.inputs():
            if v.act != L.ACT_NONE or len(v.consumers) != 1:
                raise NotImplementedError("Attn2Op inputs must be plain linear outputs with this op as sole consumer")
            plan.grad_of(v)
            _claim(v)
        d = self._desc(plan, (self.out.grad, [[v.grad for v in tok] for tok in self.tokens]))
        return [(L.load().mml_attn2_bwd, (C.byref(d),), dict(kernel="attn2_bwd_kernel", bytes=4.0 * plan.B * 14 * self.out.n))]


class JoinOp(Op):
    """parts[j] are column slices of whole.buf (torch.cat of the reference done by writing in place, e.g.
    model/cross_stitch.py:18): no launch; on the way back the parts' gradients ARE the column slices of whole.grad."""

    def __init__(self, parts, whole):
        self.parts, self.whole = parts, whole
        off = 0
        for v in parts:
            if v.buf.data_ptr() != whole.buf[:, off:off + v.n].data_ptr() or v.buf.stride(0) != whole.buf.stride(0):
                raise L.MMLError("JoinOp: part is not the expected column slice of the whole")
            if v.act != whole.act:
                raise L.MMLError("JoinOp: parts and whole must carry the same activation")
            off += v.n

    def inputs(self):
        return list(self.parts)

    def outputs(self):
        return [self.whole]

    def fwd_calls(self, plan):
        return []

    def bwd_calls(self, plan):
        if self.whole.grad is None:
            return []
        off = 0
        for v in self.parts:
            v.grad = self.whole.grad[:, off:off + v.n]
            v.deriv_applied = True  # Plan.finish / the consumer's dgrad has applied act' on the whole already
            v.written = 1
            off += v.n
        return []


class SplitOp(Op):
    """The inverse: parts[j] are column slices of whole (torch slicing, model/cross_stitch.py:22-27); their gradient
    buffers are slices of whole.grad from the start, so consumers write straight into it."""

    def __init__(self, plan, whole, widths):
        self.whole, self.parts = whole, []
        if plan.training and whole.needs_grad:
            plan.grad_of(whole)
        off = 0
        for j, w in enumerate(widths):
            v = Val(whole.buf[:, off:off + w], L.ACT_NONE, whole.needs_grad, f"{whole.name}.{j}")
            if whole.grad is not None:
                v.grad = whole.grad[:, off:off + w]
            self.parts.append(v)
            off += w

    def inputs(self):
        return [self.whole]

    def outputs(self):
        return list(self.parts)

    def fwd_calls(self, plan):
        return []

    def bwd_calls(self, plan):
        if any(v.written for v in self.parts):
            if not all(v.written for v in self.parts):
                raise L.MMLError("SplitOp: every slice needs a consumer that writes its gradient")
            self.whole.written = 1
        else:
            self.whole.grad = None
        return []


def _flat_numel(vals):
    """The flat kernels run over whole buffers: contiguous [B, n], or rows of one common zero-padded pitch."""
    if all(v.buf.is_contiguous() for v in vals):
        return vals[0].buf.numel()
    st = vals[0].buf.stride(0)
    if all(v.kpad == st and v.buf.stride(0) == st and v.n == vals[0].n for v in vals):
        return vals[0].buf.shape[0] * st
    raise L.MMLError("a flat product needs contiguous buffers (or one common zero-padded pitch)")


class MulBatchOp(Op):
    """out_j = a_j * b_j for several independent [B, n] products in ONE launch each way (PepNet: the gate products of
    every task of a layer, model/pepnet.py:72-78, :139-140; one launch per product before).  The backward writes each
    operand's gradient once, summed over the products it appears in (the gated input feeds every task's first layer),
    with the derivative of the activation that produced the operand folded in when this op is its only consumer.
    items: (a Val, b Val, out Val)."""

    def __init__(self, items, fwd_fused=False):
        self.items = items
        self.flat = [_flat_numel(it) for it in items]
        # True: the products themselves leave the epilogue of the GEMM that produces b (LinearGroupOp problems with mul /
        # prod and prod_bwd = "ext": K7 forward); this op only contributes the backward
        self.fwd_fused = bool(fwd_fused)
        if self.fwd_fused and len(items) <= 8:
            # A product whose forward left a GEMM's epilogue and that several gate-mode input-gradient problems read as
            # their factor h (PepNet's gated input: every task's first product) may receive its gradient as PARTS, one
            # buffer per reader, summed by this op's backward launch inside its sums of products -- instead of one buffer
            # the readers add to one after the other (four launches in a row for Amazon-8's four tasks)
            for _, _, o in items:
                o.grad_parts = []

    def inputs(self):
        return [v for a, b, _ in self.items for v in (a, b)]

    def outputs(self):
        return [o for _, _, o in self.items]

    @staticmethod
    def _descs(plan, rows):
        arr = ops.make_sumprod_descs(rows, "more than 8 products share one operand")
        plan.keep.append(arr)
        return arr

    def fwd_calls(self, plan):
        if self.fwd_fused:
            return []
        rows = []
        for (a, b, o), n in zip(self.items, self.flat):
            # the product's magnitude for the GEMMs that read it (only when the flat launch covers no padding columns)
            slot = plan.new_amax() if (o.amax is None and o.buf.stride(0) == o.n) else None
            if slot is not None:
                o.amax = slot
            rows.append((o.buf, n, [(a.buf, b.buf)], 0, L.ACT_NONE, None, slot))
        return [(L.load().mml_sumprod_batch, (self._descs(plan, rows), len(rows)),
                 dict(kernel="sumprod_batch_kernel", bytes=12.0 * sum(self.flat)))]

    def bwd_calls(self, plan):
        targets = {}  # id(operand) -> [operand, flat numel, [(dout, other factor)]]
        for (a, b, o), n in zip(self.items, self.flat):
            douts = list(getattr(o, "grad_parts", None) or [])
            if o.grad is not None:
                douts.append(o.grad)
            if not douts:
                continue
            if any(d_.stride(0) != o.buf.stride(0) for d_ in douts):
                raise L.MMLError("MulBatchOp: value / gradient pitch mismatch")
            for v, other in ((a, b), (b, a)):
                if v.needs_grad:
                    targets.setdefault(id(v), [v, n, []])[2].extend((d_, other.buf) for d_ in douts)
        rows, nbytes = [], 0.0
        for v, n, terms in targets.values():
            g = plan.grad_of(v)
            acc = _claim(v)
            fold = (not acc and v.act != L.ACT_NONE and not v.deriv_applied and len(v.consumers) == 1)
            if fold:
                v.deriv_applied = True
            # magnitude of the gradient as stored (tracked like a dgrad GEMM's amax_out): this flat launch can raise it
            # only when it covers no padding columns
            slot = plan.grad_slot(v) if g.stride(0) == v.n else None
            rows.append((g, n, terms, acc, v.act if fold else L.ACT_NONE, v.buf, slot))
            nbytes += 4.0 * n * (2 * len(terms) + 1 + (1 if (acc or fold) else 0))
        if not rows:
            return []
        return [(L.load().mml_sumprod_batch, (self._descs(plan, rows), len(rows)),
                 dict(kernel="sumprod_batch_kernel", bytes=nbytes))]


class CopyColsOp(Op):
    """dst[:, :] = src[:, :] for column-sliced views; no gradient flows (used for detached concatenations,
    model/pepnet.py:72, :139)."""

    def __init__(self, src, dst, amax_out=None):
        self.src, self.dst, self.amax_out = src, dst, amax_out

    def fwd_calls(self, plan):
        if self.amax_out is not None:
            # round 6: the copy raises the magnitude slot of the operand it assembles (mml_copy2d_desc.amax_out) -- PepNet's
            # two gate inputs cost a pass of mml_amax_batch each (17-20 us of a 1.67 ms step) right behind their copies
            return [_copy2d_batch_call(plan, [(self.src, self.dst)], amax=[self.amax_out])]
        return [plan.bound(bind.copy2d(self.src, self.dst, 0))]


class SumProdBatchOp(Op):
    """Derived parameters as ONE launch each way: out_j = sum_k x_jk * y_jk (y optional).  STAR: W_eff = W_spec * W_shared
    and b_eff = b_spec + b_shared for every head and layer (model/utils.py:214-216); the backward sums every factor's
    gradient over the items it appears in (d W_shared = sum_heads dW_eff * W_spec) -- fixed order, no atomics.
    items: (out PVal, [(x PVal, y PVal or None), ...])."""

    def __init__(self, items):
        self.items = items

    @staticmethod
    def _descs(plan, rows):
        """rows: (out, [(x, y or None), ...], accumulate) over whole tensors of one size."""
        for out, terms, _ in rows:
            if any(t.numel() != out.numel() for xy in terms for t in xy if t is not None):
                raise L.MMLError("SumProdBatchOp: operand size mismatch")
        arr = ops.make_sumprod_descs([(out, out.numel(), terms, acc, L.ACT_NONE, None) for out, terms, acc in rows],
                                     "more than 8 terms in one derived-parameter sum")
        plan.keep.append(arr)
        return arr

    def fwd_calls(self, plan):
        rows = [(out.data, [(x.data, y.data if y is not None else None) for x, y in terms], 0)
                for out, terms in self.items]
        return [(L.load().mml_sumprod_batch, (self._descs(plan, rows), len(rows)),
                 dict(kernel="sumprod_batch_kernel", bytes=12.0 * sum(o.data.numel() for o, _ in self.items)))]

    def bwd_calls(self, plan):
        grads = {}  # id(param) -> (param, [(dout, other factor or None)])
        for out, terms in self.items:
            if not out.written:
                continue
            for x, y in terms:
                for p, other in ((x, y), (y, x)):
                    if p is not None and p.needs_grad:
                        grads.setdefault(id(p), (p, []))[1].append((out.grad, other.data if other is not None else None))
        rows = [(p.grad, terms, _claim(p)) for p, terms in grads.values()]
        if not rows:
            return []
        return [(L.load().mml_sumprod_batch, (self._descs(plan, rows), len(rows)),
                 dict(kernel="sumprod_batch_kernel", side=True))]


class SnrWeightsOp(Op):
    """Routing weights of an SNR-trans / MSSM gate (model/snr_trans.py:38-50, model/mssm.py:40-58): W[o][j] =
    M[o][j] scaled by the hard-concrete z(u, alpha) -- one coefficient per block (u: PVal [No, Ne], learned) or one per
    output column (u: frozen tensor [No, Ne, units], MSSM).  views[o] are PVals over W[o] seen as the [n_in*units,
    units] ([K,N]) weight of output o's routing GEMM.  Backward turns their weight gradients into du and dalpha."""
    BETA, GAMMA, EPS = 0.9, -0.1, 1.1

    def __init__(self, u, alpha, M, W, dW, views):
        self.u, self.alpha, self.M, self.W, self.dW, self.views = u, alpha, M, W, dW, views
        self.n_blocks = M.shape[0] * M.shape[1]
        self.block = M.shape[2] * M.shape[3]
        self.u_learned = isinstance(u, PVal)
        self.u_data = u.data if self.u_learned else u
        self.zw = 1 if self.u_data.numel() == self.n_blocks else M.shape[3]
        if self.u_data.numel() != self.n_blocks * self.zw:
            raise L.MMLError("SnrWeightsOp: u must hold one coefficient per block or per block column")

    def fwd_calls(self, plan):
        return [plan.bound(bind.snr_gate_weights_fwd(self.u_data, self.alpha.data, self.M, self.W, self.n_blocks,
                                                     self.block, self.zw, self.BETA, self.GAMMA, self.EPS),
                           kernel="snr_weights_fwd_kernel", bytes=8.0 * self.W.numel())]

    def bwd_calls(self, plan):
        if not any(v.written for v in self.views):
            return []
        if not all(v.written for v in self.views):
            raise L.MMLError("SnrWeightsOp: every routing weight needs its gradient")
        du, acc_u = (self.u.grad, _claim(self.u)) if self.u_learned else (None, 0)
        return [plan.bound(bind.snr_gate_weights_bwd(self.dW, self.M, self.u_data, self.alpha.data, du, self.alpha.grad,
                                                     acc_u, _claim(self.alpha), self.n_blocks, self.block, self.zw,
                                                     self.BETA, self.GAMMA, self.EPS, plan.empty(self.n_blocks)),
                           kernel="snr_weights_bwd_kernel", bytes=8.0 * self.W.numel(), side=True)]


class PAddOp(Op):
    """Derived parameter out = sum(inputs) (STAR bias sums, model/utils.py:216)."""

    def __init__(self, ins, out):
        self.ins, self.out = ins, out

    def fwd_calls(self, plan):
        return [plan.bound(bind.ew_add_n([p.data for p in self.ins], self.out.data))]

    def bwd_calls(self, plan):
        if not self.out.written:
            return []
        return [plan.bound(bind.copy_flat(self.out.grad, p.grad, _claim(p), n=self.out.data.numel()),
                           kernel="copy2d_kernel", side=True) for p in self.ins if p.needs_grad]


# ---- PCGrad per-task step (reference model/optimizer.py:10-138; trainer.PCGradSchedule) --------------------------------
def _op_edges(op):
    """[(output Vals, input Vals, PVals)] of an op, one entry per independent problem of a grouped launch: the edges the
    reference's autograd graph would have."""
    if isinstance(op, GatherOp):
        return [([op.out], [], list(op.tables))]
    if isinstance(op, LinearGroupOp):
        edges = []
        for q in op.p:
            mul = q.get("mul")
            edges.append(([q["out"]] + ([q["prod"]] if mul is not None else []),
                          [q["x"]] + ([mul] if mul is not None else []),
                          [q["W"]] + ([q["b"]] if q.get("b") is not None else [])))
        return edges
    if isinstance(op, GateGroupOp):
        return [([g["mix"]], [op.experts[i] for i in g["expert"]] + [g["G"]], [g["Wg"]]) for g in op.gates]
    if isinstance(op, BNOp):
        return [([op.y], [op.z], [op.gamma, op.beta])]
    if isinstance(op, DropoutOp):
        return [([op.y], [op.x], [])]
    if isinstance(op, PReluBatchOp):
        return [([y], [z], [a]) for z, y, a in op.items]
    raise NotImplementedError(f"PCGrad per_task: no gradient-reach rule for {type(op).__name__}")


def pcgrad_reach(plan):
    """Per objective: the ids of the PVals (parameters, tables) that objective has a gradient for -- what the reference
    reads off `p.grad is None` after objective t's backward (model/optimizer.py:130-137) -- derived from the recorded ops
    by walking back from the heads' inputs.
    Objective t is loss(y_pred[:, t], y[:, t]) with y_pred = torch.cat(task_outs, -1) (reference model/mmoe.py:108,
    model/basemodel.py:294-296): the backward of the column slice hands the concatenation a gradient for EVERY head's
    output (zeros for the others), so autograd gives every parameter that any head reaches a gradient -- of zeros -- under
    every objective, never None.  The fixtures of tests/golden/make_golden_pcgrad.py record exactly that (has/<param> is 1
    throughout), and with it the merge takes the MEAN everywhere (model/optimizer.py:58): the sets below are the union over
    the heads.  A parameter no head reaches has no gradient under any objective and is in no set."""
    head = plan.head_op
    if type(head) is not HeadOp:
        raise NotImplementedError(f"PCGrad per_task: {type(head).__name__}")
    edges = [e for op in plan.ops for e in _op_edges(op)]
    union = set()
    for h in head.heads:
        vals = {id(h["Hin"])} | ({id(h["gate"])} if h.get("gate") is not None else set())
        pvs = {id(h[k]) for k in ("w", "bias", "bias2") if h.get(k) is not None}
        for outs, ins, params in reversed(edges):
            if any(id(o) in vals for o in outs):
                vals.update(id(v) for v in ins)
                pvs.update(id(p) for p in params)
        union |= pvs
    return [set(union) for _ in head.heads]


def pcgrad_segments(plan, store, reach, dense_bank, table_banks, marks_of):
    """The mml_pcgrad_seg list of a plan: runs of arena-adjacent MLP parameters that the same objectives reach (one flat
    segment each), then every table with its row marks.  dense_bank [T, arena]; table_banks[name] [T, V, E]; marks_of: id of
    a table's PVal -> its slice of the scatter's byte map (absent: every row is read)."""
    T = len(reach)
    arena = store.arena
    dense = sorted(((pv.grad.data_ptr() - arena.data_ptr()) // 4, pv) for pv in store.pvals.values()
                   if not pv.is_table and pv.grad is not None and pv.written)
    segs, run = [], None
    for off, pv in dense:
        has = tuple(id(pv) in reach[t] for t in range(T))
        if not any(has):
            continue
        if run is not None and run[1] == off and run[2] == has:
            run[1] = off + pv.grad.numel()
        else:
            run = [off, off + pv.grad.numel(), has]
            segs.append(run)
    out = [dict(banks=[dense_bank[t, a:b] if has[t] else None for t in range(T)], out=arena[a:b]) for a, b, has in segs]
    for n in store.table_names:
        pv = store.pvals[n]
        if not pv.written or not any(id(pv) in reach[t] for t in range(T)):
            continue
        out.append(dict(banks=[table_banks[n][t] if id(pv) in reach[t] else None for t in range(T)], out=pv.grad,
                        marks=marks_of.get(id(pv))))
    return out
