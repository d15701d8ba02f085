"""Call-list passes: what rewrites a plan's lists AFTER engine.Plan has recorded them -- the prologues in front of `fwd`,
merged copies, merged weight-gradient launches, the fused tower + head launch, merged row reductions.

Every pass is a function of the plan (or of call lists and a `keep` list) and of `lib`, the C-ABI library (default
L.load()): a pass only compares the functions' identity and reads descriptor fields, so stand-in functions drive it on a
machine without a GPU (tests/test_plan_passes_cpu.py).  The decisions inside the passes -- slab_cost, wgrad_chunks,
targets_distinct, match_tower_head, reindex_ready -- are pure functions of numbers and descriptor fields.

One rule for `ready`: a side call's `ready` tag is an index into plan.bwd (trainer._early_fork and segmented_step trust
it), so a pass that inserts, deletes or merges entries of `bwd` describes what it did as a `where` table and calls
reindex_ready.  This module imports engine; engine calls into it from Plan.finish only.
"""
import ctypes as C

import torch

from . import _lib as L
from . import bind
from . import engine as E
from . import ops
from .engine import call_meta

DELETED = None  # `where` entry of an old `bwd` entry that has no successor in the new list


def reindex_ready(side_calls, where):
    """Carries the `ready` tags of `side_calls` into the index space of a rewritten backward chain.  where[i] is the new
    index of old entry i of `bwd`, or DELETED.  ready = k says "the first k old entries have been issued", which becomes
    "everything up to the new entry that holds the last surviving one of them": where[k - 1] + 1 for a merge, k or k - 1
    around a deletion.  ready = 0 (nothing needed) stays 0; a tag past the end of the table counts as its length."""
    for c in side_calls:
        m = call_meta(c)
        k = m.get("ready")
        if k:
            live = [w for w in where[:k] if w is not DELETED]
            m["ready"] = live[-1] + 1 if live else 0


# ---- prologues: the entries in front of the first op's calls (Plan.prepend keeps n_pre) ---------------------------------
def cast16_prologue(plan, lib=None):
    """bf16-storage path: the bf16 copies of the weights, ONE launch in front of everything else; and the promise
    behind every bf16 value -- only bf16-storage layer groups read it -- is checked."""
    for op in list(plan.ops) + [getattr(plan, "head_op", None)]:
        for v in (op.inputs() if op is not None else []):
            if isinstance(v, E.Val) and v.is16 and isinstance(op, E.GateGroupOp) and any(v is e for e in op.experts):
                continue  # (the fast gate kernels read bf16 expert outputs: mml_gate_group.out_bf16 bit 3)
            if isinstance(v, E.Val) and v.is16 and not (isinstance(op, E.LinearGroupOp) and op.use16):
                raise L.MMLError(f"bf16 value {v.name!r} is read by {type(op).__name__}: only bf16-storage layer "
                                 "groups may read a store16 value")
    if not plan.cast16_items or plan.cast16_pre_done:
        return
    lib = lib or L.load()
    arr = ops.make_cast16_descs(plan.cast16_items)
    plan.keep.append(arr)
    n = sum(w.numel() for w, _, _ in plan.cast16_items)
    plan.prepend([(lib.mml_cast16_batch, (arr, len(plan.cast16_items)), dict(kernel="cast16_kernel", bytes=6.0 * n))])
    plan.cast16_pre_done = True


def amax_prologue(plan, lib=None):
    """Zero EVERY magnitude slot of the plan (forward and backward ones: the producers only ever raise them) and
    measure the stable weights, as the first entries of `fwd`.  Called when the whole plan has been recorded."""
    if plan.amax_pool is None or not plan.amax_next or plan.amax_pre_done:
        return
    lib = lib or L.load()
    reset = bind.amax_reset(plan.amax_pool, plan.amax_next)
    pre = [(getattr(lib, reset.name), reset.args, dict(kernel="amax_reset", bytes=32.0 * plan.amax_next))]
    cut = []
    if plan.planes_items:  # (after the magnitudes of the weights: the cut reads them)
        arr = ops.make_planes_descs(plan.planes_items)
        plan.keep.append(arr)
        cut.append((lib.mml_gemm_planes_cut, (arr, len(plan.planes_items)),
                    dict(kernel="planes_cut_kernel", bytes=8.0 * sum((it[0][0] if isinstance(it[0], tuple) else it[0]).numel()
                                                                    for it in plan.planes_items))))
    # The weights' magnitudes ride in the magnitude launch that stands in front of the first GEMM anyway (the pass over
    # the gathered input): one launch fewer at the head of the step (~6 us of a 1.7 ms step).  Nothing in front of the
    # first GEMM reads a weight's slot or planes.  MMLREC_AMAX_MERGE=0: the separate launch of round 3.
    first_gemm = next((i for i, c in enumerate(plan.fwd) if c[0] in (lib.mml_gemm_grouped_fwd, lib.mml_pep_gate_fwd)),
                      len(plan.fwd))
    host = next((i for i, c in enumerate(plan.fwd[:first_gemm]) if c[0] is lib.mml_amax_batch and
                 "need" in call_meta(c)), None)
    if plan.amax_wlist and host is not None and plan.knobs.amax_merge:
        c = plan.fwd[host]
        merged = plan.amax_call(call_meta(c)["need"] + plan.amax_wlist, lib=lib,
                                **{k: v for k, v in call_meta(c).items() if k not in ("kernel", "bytes", "need")})
        plan.fwd = plan.fwd[:host] + [merged] + cut + plan.fwd[host + 1:]
    else:
        if plan.amax_wlist:
            pre.append(plan.amax_call(plan.amax_wlist, lib=lib))
        pre += cut
    plan.prepend(pre)
    plan.amax_pre_done = True


# ---- merged copies ------------------------------------------------------------------------------------------------------
def merge_copies(calls, keep, lib=None, where=None):
    """Runs of neighbouring strided copies (mml_copy2d / mml_copy2d_batch: concat / split of feature blocks, gradient
    hand-overs of shared parameters) as ONE launch each -- inside a step's graph every launch takes >= 4.6 us from
    start to end, and PepNet's step had four of them in a row three times.  A copy joins the run only if it touches
    nothing an earlier copy of the run writes, and writes nothing an earlier one reads (one launch has no order).
    keep: receives the descriptor arrays of the merged launches.
    where: a list that receives, per input call, the index of the output entry it went into."""
    lib = lib or L.load()  # (tests/test_plan_passes_cpu.py passes stand-ins: only the functions' identity is used)
    f1, fb = lib.mml_copy2d, lib.mml_copy2d_batch

    def descs_of(c):
        if c[0] is f1:
            src, lds, dst, ldd, rows, cols, acc = c[1]
            return [(src, lds, dst, ldd, rows, cols, acc, None)]
        arr, n = c[1]
        # (the 8th entry: an item's optional magnitude slot, mml_copy2d_desc.amax_out -- stand-in arrays of the CPU
        #  tests need not have the field)
        return [(arr[k].src, arr[k].lds, arr[k].dst, arr[k].ldd, arr[k].rows, arr[k].cols, arr[k].accumulate,
                 getattr(arr[k], "amax_out", None)) for k in range(n)]

    def span(ptr, ld, rows, cols):
        return (ptr, ld, rows, cols)

    def hits(a, b):
        """Do the [rows, cols] regions a, b (pointer, pitch, rows, cols; float32) share an element?  Exact for regions of
        one pitch (column blocks of one buffer: the concat / split case), the byte-interval test otherwise."""
        (pa, la, ra, ca), (pb, lb, rb, cb) = a, b
        ea, eb = pa + 4 * ((max(ra, 1) - 1) * la + ca), pb + 4 * ((max(rb, 1) - 1) * lb + cb)
        if not (pa < eb and pb < ea):
            return False
        if la == lb and la > 0 and (pb - pa) % 4 == 0:
            delta = (pb - pa) // 4
            q, r = divmod(delta, la)   # b's origin in a's grid: row q, column r (Python's floor semantics)
            if ca <= la and r + cb <= la:
                rows_meet = q < ra and q + rb > 0
                cols_meet = r < ca and r + cb > 0
                return rows_meet and cols_meet
        return True

    out, run, meta_run = [], [], []
    pos = [0] * len(calls)
    run_src = []

    def flush():
        if not run:
            return
        for i_ in run_src:
            pos[i_] = len(out)
        run_src.clear()
        if len(meta_run) == 1:
            out.append(meta_run[0])
        else:
            arr = (L.Copy2dDesc * len(run))()
            for d, (src, lds, dst, ldd, rows, cols, acc, am) in zip(arr, run):
                d.src, d.lds, d.dst, d.ldd, d.rows, d.cols, d.accumulate = src, lds, dst, ldd, rows, cols, acc
                if am:
                    d.amax_out = am
            keep.append(arr)
            meta = dict(kernel="copy2d_batch_kernel",
                        bytes=sum(8.0 * r[4] * r[5] for r in run))
            for c in meta_run:  # (the scheduling tags of the merged calls: they were neighbours of ONE list)
                m = call_meta(c)
                for k in ("side", "tail", "rank", "ready"):
                    if k in m:
                        meta[k] = max(meta.get(k, m[k]), m[k]) if k == "ready" else m[k]
            out.append((fb, (arr, len(run)), meta))
        run.clear()
        meta_run.clear()

    for ci, c in enumerate(calls):
        if c[0] is f1 or c[0] is fb:
            ds = descs_of(c)
            ok = len(run) + len(ds) <= 32
            for (src, lds, dst, ldd, rows, cols, acc, _am) in ds:
                rs, ws = span(src, lds, rows, cols), span(dst, ldd, rows, cols)
                for (s2, l2, d2, ld2, r2, c2, a2, _am2) in run:
                    rs2, ws2 = span(s2, l2, r2, c2), span(d2, ld2, r2, c2)
                    if hits(rs, ws2) or hits(ws, rs2) or hits(ws, ws2):
                        ok = False
            if not ok:
                flush()
            run.extend(ds)
            meta_run.append(c)
            run_src.append(ci)
        else:
            flush()
            pos[ci] = len(out)
            out.append(c)
    flush()
    if where is not None:
        where[:] = pos
    return out


def merge_plan_copies(plan, lib=None):
    """merge_copies over every list of a recorded plan (MMLREC_MERGE_COPIES=0: off)."""
    if not plan.knobs.merge_copies:
        return
    for name in ("fwd", "bwd", "bwd_tail", "bwd_side", "head_train", "head_bwd"):
        where = [] if name == "bwd" else None
        setattr(plan, name, merge_copies(getattr(plan, name), plan.keep, lib=lib, where=where))
        if name == "bwd" and where:
            # the side calls' `ready` tags count entries of the UNMERGED chain: into the merged list's index
            # space (ready = k: the first k entries have been issued -> everything up to the merged entry that
            # holds old entry k - 1)
            reindex_ready(list(plan.bwd_side) + list(plan.head_side), where)


# ---- merged weight-gradient launches ------------------------------------------------------------------------------------
def slab_cost(tiles, steps, slab_div, slab_cap):
    """Batch steps a launch of `tiles` 128 x 128 output tiles takes over `steps` steps of the batch: the batch is cut into
    slabs (at most steps // slab_div of them, at most slab_cap) so that tiles x slabs fill the chip's 512 workgroup slots
    once; a launch + reduction pair is priced at ~8 steps on top."""
    sl = max(1, min(512 // max(tiles, 1), steps // slab_div, slab_cap))
    return -(-steps // sl) * -(-tiles * sl // 512) + 8


def targets_distinct(descs):
    """Every problem writes a dW / dbias of its own and nobody accumulates: the problems may share a launch (a weight
    shared by two layers is written by two launches in order)."""
    targets = [d.dW for d in descs] + [d.dbias for d in descs if d.dbias]
    return len(set(targets)) == len(targets) and not any(d.accumulate for d in descs)


def wgrad_chunks(shapes, serves, B, nt_group):
    """merge_wgrad's decision at B >= 16 384.  shapes: per recorded launch the (N, K) of its problems; serves: per problem,
    in that order, whether gemm_nt_kernel takes it; nt_group: problems per gemm_nt_kernel launch.  Returns the merged
    launches as lists of problem numbers, or None where the per-layer launches take no more steps."""
    # Large batches (gemm_nt_kernel: 128 x 128 output tiles, the batch cut into `slabs` pieces so that tiles x
    # slabs fill the chip's 512 workgroup slots once; at most MML_MAX_GROUP problems per launch): merge when the
    # merged launches take fewer batch steps than the per-layer launches together, a launch + reduction pair
    # priced at ~8 steps.  AE-30: 20 / 8 / 2 tiles -> 82 + 32 + 32 steps per layer against 121 merged (measured
    # 1.65 -> 1.565 ms); KuaiRec-32: 72 / 32 / 4 tiles -> 293 + 128 + 32 against 512 merged (108 tiles x 4 slabs
    # leave 80 slots idle: 3.33 -> 3.38 ms merged, so it stays per layer); PepNet's 40-odd small problems go
    # into launches of 16 (2.21 -> 2.13 ms already as ONE call that fell to the tile kernel).
    steps = B // 32
    flat = [s for g in shapes for s in g]
    # (what gemm_nt_kernel takes -- csrc/gemm_route.hpp, nt_serves -- goes together: ONE problem it does
    # not take, e.g. a final layer with a single output row, would send its whole launch to the tile kernel)
    fits = [i for i, ok in enumerate(serves) if ok]
    other = [i for i, ok in enumerate(serves) if not ok]
    chunks = []
    for part, cap in ((fits, nt_group), (other, L.MAX_GROUP)):
        if part:
            nch = -(-len(part) // cap)
            per = -(-len(part) // nch)
            chunks += [part[i:i + per] for i in range(0, len(part), per)]

    def cost(g):
        return slab_cost(sum(-(-N // 128) * -(-K // 128) for N, K in g), steps, 8, 64)

    if sum(cost([flat[i] for i in ch]) for ch in chunks) >= sum(cost(g) for g in shapes):
        return None
    return chunks


def _phase_pair(fn, size_fn, descs, device, keep, meta, reduce_kernel, min_ws=0):
    """The (partial products, reduction) entries of ONE phased weight-gradient launch over copies of `descs`: the
    descriptors cloned into a fresh array, the workspace the library asks for allocated, both kept alive in `keep`."""
    arr = (type(descs[0]) * len(descs))()
    for k, d in enumerate(descs):
        C.memmove(C.byref(arr[k]), C.byref(d), C.sizeof(d))
    nbytes = int(size_fn(arr, len(descs)))
    if nbytes < 0:
        L.check(-1, getattr(size_fn, "__name__", "workspace_bytes"))
    ws = torch.empty(max(nbytes, min_ws), dtype=torch.uint8, device=device)
    keep += [arr, ws]
    args = (arr, len(descs), ws.data_ptr(), ws.numel())
    return ((fn, args + (1,), meta),
            (fn, args + (2,), dict(kernel=reduce_kernel, bytes=float(nbytes), side=True, rank=1)))


def merge_wgrad(plan, lib=None):
    """Small batches: every weight-gradient GEMM of the step in ONE grouped launch (+ one reduction) instead of one
    pair per layer.  At M = 4 096 a layer's launch fills a fraction of the chip for ~15 us; together they take the
    time of the longest (lazy_exact step on AE-30: 0.327 -> see DESIGN 10.12).  Only when every problem writes its
    own dW (a weight shared by two layers is written by two launches in order).  At large batches the per-layer
    order stays: each launch fills the chip by itself and the reductions interleave with the next GEMM."""
    lib = lib or L.load()
    fn = lib.mml_gemm_grouped_wgrad_phase
    idx = [i for i, c in enumerate(plan.bwd_side) if c[0] is fn]
    if len(idx) <= 2:
        return False
    # the partial-product phase carries the problems (phase 2 repeats them)
    groups = [[c[1][0][k] for k in range(c[1][1])] for c in (plan.bwd_side[i] for i in idx) if c[1][4] == 1]
    descs = [d for g in groups for d in g]
    chunks = [descs]  # (small batches: ONE call, the library splits it into groups of MML_MAX_GROUP for the tile kernel)
    if plan.B >= 16384:
        serves = [bool(lib.mml_gemm_nt_serves(C.byref(d))) for d in descs]  # (the library's own predicate)
        # (round 6: gemm_nt_kernel takes 48 problems per launch; MMLREC_NT_GROUP=16 restores the launches of round 5)
        picked = wgrad_chunks([[(d.N, d.K) for d in g] for g in groups], serves, plan.B, plan.knobs.nt_group)
        if picked is None:
            return False
        chunks = [[descs[i] for i in ch] for ch in picked]
    if not targets_distinct(descs):
        return False
    flops = sum(call_meta(plan.bwd_side[i]).get("flops", 0.0) for i in idx)
    hbm = sum(call_meta(plan.bwd_side[i]).get("hbm_bytes", 0.0) for i in idx)
    pairs = []
    for ch in chunks:
        share = len(ch) / float(len(descs))
        pairs.append(_phase_pair(fn, lib.mml_gemm_grouped_wgrad_workspace_bytes, ch, plan.device, plan.keep,
                                 dict(kernel=E._gemm_symbol(False, False, [], 2), flops=flops * share,
                                      hbm_bytes=hbm * share, side=True, rank=0), "slab_reduce"))
    rest = [c for i, c in enumerate(plan.bwd_side) if i not in set(idx)]  # (un-padding copies: after the reduction)
    # (each reduction right behind its launch: the next launch's first tiles start beside it)
    plan.bwd_side = [c for pair in pairs for c in pair] + rest
    return True


def merge_wgrad16(plan, lib=None):
    """bf16-storage path (csrc/gemm16.hip: mml_g16_wgrad, at most G16_MAX_GROUP problems per launch, 128 x 128 tiles
    of 64-row steps, at most 32 slabs): neighbouring weight-gradient launches go together where the tile model says
    the merged launch takes fewer steps -- KuaiRec-32: towers (4 tiles -> 128 workgroups for 512 slots) + second
    expert layers (32 tiles) as one launch of 36 tiles."""
    lib = lib or L.load()
    fn = lib.mml_g16_wgrad
    side = plan.bwd_side
    idx = [i for i, c in enumerate(side) if c[0] is fn and c[1][4] == 1]
    if len(idx) < 2 or any(side[i + 1][0] is not fn or side[i + 1][1][4] != 2 for i in idx):
        return False
    steps = max(plan.B // 64, 1)

    def cost(g):
        return slab_cost(sum((d.N // 128) * (d.K // 128) for d in g), steps, 4, 32)

    groups = [[side[i][1][0][k] for k in range(side[i][1][1])] for i in idx]
    metas = [call_meta(side[i]) for i in idx]
    out, om = [groups[0]], [dict(metas[0])]
    for g, m in zip(groups[1:], metas[1:]):
        cur = out[-1]
        if (len(cur) + len(g) <= L.G16_MAX_GROUP and cost(cur + g) < cost(cur) + cost(g) and
                targets_distinct(cur + g)):
            out[-1] = cur + g
            for k in ("flops", "hbm_bytes"):
                om[-1][k] = om[-1].get(k, 0.0) + m.get(k, 0.0)
        else:
            out.append(g)
            om.append(dict(m))
    if len(out) == len(groups):
        return False
    calls = []
    for g, m in zip(out, om):
        m["kernel"] = "g16_nt_kernel(wgrad %d problems)" % len(g)
        calls += _phase_pair(fn, lib.mml_g16_wgrad_workspace_bytes, g, plan.device, plan.keep, m, "g16_reduce_kernel",
                             min_ws=16)
    drop = set(idx) | {i + 1 for i in idx}
    first = idx[0]
    plan.bwd_side = ([c for i, c in enumerate(side) if i < first and i not in drop] + calls +
                     [c for i, c in enumerate(side) if i > first and i not in drop])
    return True


# ---- K5': the fused tower + head launch ---------------------------------------------------------------------------------
def match_tower_head(fwd, head_train, head_side, bwd, lib):
    """The pattern fuse_tower_head replaces, or None: a forward launch of T Linear + ReLU problems whose outputs are the T
    heads' inputs and nothing else's (fwd[fi]), the deferred head launch (head_train / head_side: one entry each), and an
    input-gradient launch of T single-source problems over the heads' dH (bwd[di]).  Returns (fi, di, [(f, d, h) per task]):
    the forward problem, the input-gradient problem and the head descriptor of task t.  Reads descriptor fields only."""
    fh, ff, fd = lib.mml_head_bce_fwd_bwd_phase, lib.mml_gemm_grouped_fwd, lib.mml_gemm_grouped_dgrad
    if len(head_train) != 1 or len(head_side) != 1:
        return None
    hc, hs = head_train[0], head_side[0]
    if hc[0] is not fh or hs[0] is not fh or hc[1][3] != 1 or hs[1][3] != 2:
        return None
    grp = hc[1][0]._obj
    T = int(grp.n_heads)
    if grp.dh_bf16 or grp.dprob or not grp.y or not grp.prob or T < 1:
        return None
    heads = [grp.head[t] for t in range(T)]
    if any(h.gate or h.w2 or not h.dH or not h.h_relu or not h.dw or not h.dbias for h in heads):
        return None
    hin = {int(h.Hin): t for t, h in enumerate(heads)}
    dh = {int(h.dH): t for t, h in enumerate(heads)}
    if len(hin) != T or len(dh) != T:
        return None
    # the forward launch that writes the heads' inputs
    fi = next((i for i in range(len(fwd) - 1, -1, -1) if fwd[i][0] is ff and fwd[i][1][1] == T and
               all(int(fwd[i][1][0][k].C or 0) in hin for k in range(T))), None)
    # the input-gradient launch over the heads' dH
    di = next((i for i, c in enumerate(bwd) if c[0] is fd and c[1][1] == T and
               all(c[1][0][k].n_src == 1 and int(c[1][0][k].dC[0] or 0) in dh for k in range(T))), None)
    if fi is None or di is None:
        return None
    fdesc, ddesc = fwd[fi][1][0], bwd[di][1][0]
    by_t_f = {hin[int(fdesc[k].C)]: fdesc[k] for k in range(T)}
    by_t_d = {dh[int(ddesc[k].dC[0])]: ddesc[k] for k in range(T)}
    if len(by_t_f) != T or len(by_t_d) != T:
        return None
    for t in range(T):
        f, d, h = by_t_f[t], by_t_d[t], heads[t]
        if (f.act != L.ACT_RELU or f.w_kn or f.mul or not f.w_planes or not f.w_kexp or not f.amax_a or f.M != int(grp.B) or
                f.N != h.H or int(f.ldc) != int(h.ldh)):
            return None
        if (d.gate_h or d.Y or d.relu_mask or d.act != L.ACT_NONE or d.accumulate or d.w_kn[0] or not d.w_planes[0] or
                not d.w_kexp[0] or not d.dA or d.K != f.K or d.N[0] != f.N or int(d.W[0] or 0) != int(f.W or 0) or
                int(d.lddc[0]) != int(h.lddh)):
            return None
    return fi, di, [(by_t_f[t], by_t_d[t], heads[t]) for t in range(T)]


def build_tower_head(grp, tasks):
    """The mml_tower_head_group of a matched pattern: grp = the heads' mml_head_group, tasks = match_tower_head's (f, d, h)."""
    g = L.TowerHeadGroup()
    g.n, g.M = len(tasks), int(grp.B)
    g.prob, g.ldprob, g.y, g.ldy, g.mask, g.ldmask, g.loss = grp.prob, grp.ldprob, grp.y, grp.ldy, grp.mask, grp.ldmask, grp.loss
    for t, (f, d, h) in enumerate(tasks):
        q = g.t[t]
        q.A, q.lda, q.amax_a, q.K, q.N = f.A, f.lda, f.amax_a, f.K, f.N
        q.w_planes_fwd, q.ldpf, q.kexp_fwd = f.w_planes, f.ldw, f.w_kexp
        q.w_planes_bwd, q.ldpb, q.kexp_bwd = d.w_planes[0], d.ldw[0], d.w_kexp[0]
        q.bias1, q.w, q.hbias, q.hbias2, q.n_hbias2 = f.bias, h.w, h.bias, h.bias2, h.n_bias2
        q.dH, q.lddh, q.dA, q.ldda, q.dw, q.dhbias = h.dH, h.lddh, d.dA, d.ldda, h.dw, h.dbias
        q.amax_dH, q.amax_dA = grp.amax_dH, d.amax_out
        q.mask_col, q.head, q.kind = h.mask_col, t, h.kind
    return g


def fuse_tower_head(plan, lib=None):
    """K5' (csrc/tower_head.hip): the last tower layer of every task, the heads + summed BCE and the towers' input gradient
    -- three launches of the recorded step -- as ONE launch (+ its share of the batched reduction), when the recorded
    lists hold exactly that pattern (match_tower_head).  Rewrites fwd / head_train / head_side / bwd of THIS plan (a
    TrainStep's own: the forward-only and the dL/dprob lists of a model's cached plans are never touched).
    MMLREC_TOWER_HEAD=0: off.
    Afterwards `fwd` no longer writes the heads' input, which head_infer and head_bwd still read: plan.tower_head marks
    the plan, and Plan.run_forward / run_backward_from_dprob refuse it (run_train_fwd_bwd stays valid)."""
    if not plan.knobs.tower_head or plan.amax_pool is None or plan.bf16 or plan.device.type != "cuda":
        return False
    lib = lib or L.load()
    found = match_tower_head(plan.fwd, plan.head_train, plan.head_side, plan.bwd, lib)
    if found is None:
        return False
    fi, di, tasks = found
    g = build_tower_head(plan.head_train[0][1][0]._obj, tasks)
    if not lib.mml_tower_head_serves(C.byref(g)):
        return False
    nws = int(lib.mml_tower_head_workspace_bytes(C.byref(g)))
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=plan.device)
    plan.keep += [g, ws]
    T, K, N = int(g.n), int(g.t[0].K), int(g.t[0].N)
    byts = 4.0 * g.M * T * (2 * K + N + 3)
    fused = (lib.mml_tower_head_fwd_bwd, (C.byref(g), ws.data_ptr(), ws.numel(), 1),
             dict(kernel="tower_head_kernel", bytes=byts, hbm_bytes=byts))
    red = (lib.mml_tower_head_fwd_bwd, (C.byref(g), ws.data_ptr(), ws.numel(), 2),
           dict(kernel="slab_reduce", bytes=float(nws), side=True, rank=1, ready=0))
    n_bwd = len(plan.bwd)
    del plan.fwd[fi]
    del plan.bwd[di]
    # (`ready` counts entries of the backward chain: entry di is gone, the ones behind it moved up by one)
    reindex_ready(list(plan.bwd_side) + list(plan.head_side),
                  list(range(di)) + [DELETED] + list(range(di, n_bwd - 1)))
    plan.head_train = [fused]
    plan.head_side = [red]
    plan.tower_head = g
    return True


# ---- merged row reductions ----------------------------------------------------------------------------------------------
def merge_row_reduces(plan, lib=None):
    """The deferred reductions of the head / gate kernels' partial sums (`head_side`, and the gate groups' entries of
    `bwd_side`: only the optimizer and the host read their results) as ONE launch in front of the weight gradients
    (as few as the launch's segment capacity allows)."""
    lib = lib or L.load()  # (tests/test_plan_passes_cpu.py passes stand-ins: only the functions' identity is used)
    fh, fg = lib.mml_head_bce_fwd_bwd_phase, lib.mml_gate_mix_bwd_phase
    ft = getattr(lib, "mml_tower_head_fwd_bwd", None)  # (K5': fuse_tower_head)
    is_red = lambda c: c[0] in (fh, fg, ft) and c[0] is not None and c[1][3] == 2  # noqa: E731
    picked = [c for c in list(plan.head_side) + list(plan.bwd_side) if is_red(c)]
    if len(picked) < 2:
        return False

    def segments(c):
        """Reduction segments the C side makes of this item (csrc/gate_head.hip, phase 2): a head group one per dw and
        dbias of every head plus the loss, a gate group one per active gate's dWg."""
        g = c[1][0]._obj
        if c[0] is fh:
            return 2 * int(g.n_heads) + (1 if g.loss else 0)
        if c[0] is ft:
            return 2 * int(g.n) + (1 if g.loss else 0)
        return sum(1 for k in range(int(g.n_gates)) if g.gate[k].active)

    # one launch takes at most MAX_REDUCE_SEGS segments (csrc/reduce.hpp): a deep PLE (7 tasks x 4 levels: 15 + 8 + 8 +
    # 8 + 7 = 46) goes into as many launches as it needs, in list order
    chunks, cur, nseg = [], [], 0
    for c in picked:
        s = segments(c)
        if s > L.MAX_REDUCE_SEGS:
            return False  # (a single group beyond the launch's capacity: leave every reduction where it was)
        if cur and nseg + s > L.MAX_REDUCE_SEGS:
            chunks.append(cur)
            cur, nseg = [], 0
        cur.append(c)
        nseg += s
    chunks.append(cur)
    calls = []
    for ch in chunks:
        if len(ch) == 1:  # (nothing to merge it with: its own phase-2 call, on the side list)
            calls.append(ch[0])
            continue
        items = (L.RowsReduceItem * len(ch))()
        for it, c in zip(items, ch):
            grp, ws, nbytes, _ = c[1]
            it.kind = (L.ROWS_REDUCE_HEAD if c[0] is fh else
                       (L.ROWS_REDUCE_TOWER_HEAD if c[0] is ft else L.ROWS_REDUCE_GATE))
            it.group = C.addressof(grp._obj)  # (the ops pass C.byref(group); the group itself lives in plan.keep)
            it.workspace, it.workspace_bytes = ws, nbytes
        plan.keep.append(items)
        # (no reindex_ready here: this merges SIDE calls and leaves `bwd` as it is -- the merged launch may start once the
        # latest of its items may, hence the max of their tags)
        calls.append((lib.mml_rows_reduce_batch, (items, len(ch)),
                      dict(kernel="slab_reduce", bytes=sum(call_meta(c).get("bytes", 0.0) for c in ch), side=True, rank=1,
                           ready=max(call_meta(c).get("ready", 0) for c in ch))))
    plan.head_side = [c for c in plan.head_side if not is_red(c)]
    plan.bwd_side = calls + [c for c in plan.bwd_side if not is_red(c)]
    return True
