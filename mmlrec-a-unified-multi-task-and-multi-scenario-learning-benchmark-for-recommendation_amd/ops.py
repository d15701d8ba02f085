"""Thin torch-tensor front end of the C ABI (include/mmlrec.h): argument marshalling only, no arithmetic.

torch is used for device memory and the current HIP stream; every number is produced by libmmlrec_hip.so.
All functions require CUDA(HIP) tensors and raise MMLError otherwise -- there is no CPU fallback.
"""
import ctypes as C

import os

import torch

from . import _lib as L
from . import bind

_workspaces = {}
_ld, _ptr_array = bind.ld, bind.ptr_array


def _stream():
    return torch.cuda.current_stream().cuda_stream


_masked_streams = {}


def cu_range_stream(device, cu_lo, cu_hi):
    """torch view of a HIP stream confined to compute units [cu_lo, cu_hi) (mml_stream_create_cu_range); one per
    (device, range), kept for the life of the process."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, int(cu_lo), int(cu_hi))
    st = _masked_streams.get(key)
    if st is None:
        h = C.c_void_p()
        L.check(L.load().mml_stream_create_cu_range(idx, int(cu_lo), int(cu_hi), C.byref(h)))
        st = torch.cuda.ExternalStream(h.value, device=torch.device("cuda", idx))
        _masked_streams[key] = st
    return st


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise L.MMLError("mmlrec_amd ops need tensors on an MI355X (got a CPU tensor); there is no CPU fallback")


def _f32_2d(t, name):
    if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise L.MMLError(f"{name}: expected a float32 2-D tensor with unit inner stride, got {t.dtype} {tuple(t.shape)} "
                         f"strides {t.stride()}")
    return t


def _issue(b):
    """Launch a bind.Bound on the current stream."""
    L.check(getattr(L.load(), b.name)(*b.args, _stream()), b.name)


_SPIN_CAL = {}  # device index -> (spin ticks for ~0.2 ms, measured ms of one such spin)


def concurrent_stream(device, tries=6):
    """A stream whose kernels really run beside those of the current stream.  HIP hands streams one of a few
    hardware queues round-robin (four by default); a process that also holds RCCL's streams and the routing stream of
    the row-sharded tables can find its side stream on the SAME queue as the main stream, and the forked tail then
    runs one launch after the other (seen in the kernel trace of the forced row-sharded step: weight-gradient GEMMs
    and table update on one queue, 2.10 ms where the unsharded step takes 1.88).  So: probe -- a spin kernel on each
    stream, concurrent if the pair takes the time of one -- and keep the first candidate that passes.
    MMLREC_SIDE_PROBE=0 takes the first stream unprobed."""
    main = torch.cuda.current_stream(device)
    first = torch.cuda.Stream(device=device)
    if os.environ.get("MMLREC_SIDE_PROBE", "1") == "0" or not hasattr(torch.cuda, "_sleep"):
        return first
    try:
        def timed(fn):
            torch.cuda.synchronize(device)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(main)
            fn()
            b.record(main)
            torch.cuda.synchronize(device)
            return a.elapsed_time(b)

        # torch.cuda._sleep counts s_memtime ticks (a 100 MHz constant clock on gfx9, not shader cycles): the spin length
        # for ~0.2 ms is MEASURED once per device and cached (400 000 ticks were ~4 ms per probe)
        key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
        cal = _SPIN_CAL.get(key)
        if cal is None:
            torch.cuda._sleep(1000)  # (loads the spin kernel)
            probe = 20_000
            ms = max(timed(lambda: torch.cuda._sleep(probe)), 1e-3)
            spin = int(min(max(probe * 0.2 / ms, 2_000), 2_000_000))
            one = timed(lambda: torch.cuda._sleep(spin))
            cal = _SPIN_CAL[key] = (spin, one)
        spin, one = cal

        def pair_ms(s):
            j = torch.cuda.Event()

            def both():
                a0 = torch.cuda.Event()
                a0.record(main)
                s.wait_event(a0)
                with torch.cuda.stream(s):
                    torch.cuda._sleep(spin)
                    j.record(s)
                torch.cuda._sleep(spin)
                main.wait_event(j)
            return timed(both)

        cand = first
        for _ in range(tries):
            if min(pair_ms(cand), pair_ms(cand)) < 1.5 * one:
                return cand
            cand = torch.cuda.Stream(device=device)
    except Exception:  # (a probe must never cost the step)
        pass
    return first


def workspace(nbytes, device):
    """Grow-only scratch buffer per device (kept alive here; kernels only see the raw pointer)."""
    key = (device.type, device.index)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def new_status(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


def check_status(status, what="embedding lookup"):
    """Turn the device status word into the exception nn.Embedding raises on CPU (IndexError)."""
    v = int(status.item())
    if v:
        status.zero_()
        raise IndexError(f"index out of range in {what} (status bits {v:#x}: 1 = negative, 2 = >= vocabulary)")


# ---------------------------------------------------------------------------------------------- K1 / K2
def gather_fwd(tables, X, cols, dense_col0=0, nd=0, out=None, status=None):
    """dnn_input = concat_f table_f[X[:, cols[f]].long()] ++ X[:, dense_col0:dense_col0+nd]."""
    _need_gpu(X, *tables)
    X = _f32_2d(X, "X")
    if out is None:
        out = torch.empty((X.shape[0], len(tables) * tables[0].shape[1] + nd), dtype=torch.float32, device=X.device)
    _issue(bind.gather_fwd(tables, X, cols, dense_col0, nd, out, status))
    return out


def gather_fwd_wgmax(tables, X, cols, dense_col0=0, nd=0, out=None, status=None):
    """gather_fwd that also returns the per-workgroup maxima of |out| (include/mmlrec.h: mml_gather_fwd_wgmax)."""
    lib = L.load()
    _need_gpu(X, *tables)
    X = _f32_2d(X, "X")
    F, E, B = len(tables), tables[0].shape[1], X.shape[0]
    if out is None:
        out = torch.empty((B, F * E + nd), dtype=torch.float32, device=X.device)
    n = int(lib.mml_gather_wgmax_len(F, E, nd, B))
    wg = torch.full((1, max(n, 1)), float("nan"), dtype=torch.float32, device=X.device)
    _issue(bind.gather_fwd_wgmax(tables, X, cols, dense_col0, nd, out, wg, n, status))
    return out, wg


def gather_fwd_idx32(tables, idx, dense=None, out=None, status=None):
    _need_gpu(idx, *tables)
    F, E, B = len(tables), tables[0].shape[1], idx.shape[0]
    nd = 0 if dense is None else dense.shape[1]
    if out is None:
        out = torch.empty((B, F * E + nd), dtype=torch.float32, device=idx.device)
    _issue(bind.gather_fwd_idx32(tables, idx, dense, out, status))
    return out


# ---------------------------------------------------------------------------------------------- K1p / K2p
class PooledField:
    """A multi-valued sparse feature as the kernels see it: `maxlen` id columns of X from `col0`, pooled by `combiner`
    ("sum" / "mean" / "max") over the valid positions -- ids != 0 (len_col None: mask mode) or the first X[:, len_col]
    positions (length mode) -- with the rows of table number `table`."""
    __slots__ = ("col0", "maxlen", "combiner", "table", "len_col")

    def __init__(self, col0, maxlen, combiner, table, len_col=None):
        if combiner not in L.POOL_COMBINERS:
            raise ValueError(f"combiner {combiner!r}: expected one of {sorted(L.POOL_COMBINERS)}")
        self.col0, self.maxlen, self.combiner, self.table = int(col0), int(maxlen), combiner, int(table)
        self.len_col = None if len_col is None else int(len_col)


def make_pool_desc(tables, singles, pooled, vocab=None):
    """mml_pool_desc (include/mmlrec.h): `tables` = the distinct [V, E] tensors (or None with `vocab` = (sizes, E) for
    the index-only pass), `singles` = [(X column, table number)], `pooled` = [PooledField]."""
    d = L.PoolDesc()
    if tables is not None:
        _need_gpu(*tables)
        sizes, E = [t.shape[0] for t in tables], tables[0].shape[1]
        for t in tables:
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != E or not t.is_contiguous():
                raise L.MMLError("pooled rows: every table must be a contiguous float32 [V, E] tensor of one width E")
    else:
        sizes, E = vocab
    if len(sizes) > L.MAX_FIELDS or len(pooled) > L.MAX_POOLED or len(singles) + len(pooled) > L.MAX_FIELDS:
        raise L.MMLError(f"pooled rows: at most {L.MAX_FIELDS} tables, {L.MAX_POOLED} pooled fields and "
                         f"{L.MAX_FIELDS} fields in all per launch")
    d.n_tables, d.E, d.n_single, d.n_pooled = len(sizes), int(E), len(singles), len(pooled)
    for i, v in enumerate(sizes):
        d.vocab[i] = int(v)
        d.table[i] = tables[i].data_ptr() if tables is not None else None
    for i, (c, t) in enumerate(singles):
        d.s_col[i], d.s_table[i] = int(c), int(t)
    for i, pf in enumerate(pooled):
        d.p_col0[i], d.p_maxlen[i], d.p_table[i] = pf.col0, pf.maxlen, pf.table
        d.p_len_col[i] = -1 if pf.len_col is None else pf.len_col
        d.p_combiner[i] = L.POOL_COMBINERS[pf.combiner]
    return d


def gather_pool_fwd(tables, X, singles, pooled, dense_col0=0, nd=0, out=None, argmax=None, wgmax=False, status=None):
    """dnn_input = [single-valued blocks | pooled blocks | dense columns] in ONE launch (mml_gather_pool_fwd).
    Returns (out, argmax, wg_max): argmax = uint8 [B, P * E] when a field pools by max (else None), wg_max = the
    per-workgroup maxima of |out| when wgmax is set (else None)."""
    lib = L.load()
    _need_gpu(X)
    X = _f32_2d(X, "X")
    d = make_pool_desc(tables, singles, pooled)
    B, E, P = X.shape[0], d.E, len(pooled)
    if out is None:  # rows padded to whole 16-byte pieces (the kernel stores float4s: ldo % 4 == 0)
        K0 = (len(singles) + P) * E + nd
        out = torch.empty((B, (K0 + 3) // 4 * 4), dtype=torch.float32, device=X.device)[:, :K0]
    if argmax is None and any(pf.combiner == "max" for pf in pooled):
        argmax = torch.zeros((B, P * E), dtype=torch.uint8, device=X.device)
    wg, n = None, 0
    if wgmax:
        n = int(lib.mml_gather_pool_wgmax_len(C.byref(d), nd, B))
        wg = torch.full((1, max(n, 1)), float("nan"), dtype=torch.float32, device=X.device)
    _issue(bind.gather_pool_fwd(d, X, dense_col0, nd, out, argmax, wg, n, status))
    return out, argmax, wg


def scatter_pool_bwd(grad_tables, X, singles, pooled, d_out, argmax=None, seen=None, rowbase=None, touched=None,
                     touched_count=None, status=None, marks=None):
    """Table gradients of every field, single-valued and pooled, in ONE launch (mml_scatter_pool_bwd); seen / rowbase /
    marks are per TABLE (marks: marks_bytes of the tables' sizes)."""
    _need_gpu(X, d_out)
    d = make_pool_desc(grad_tables, singles, pooled)
    _issue(bind.scatter_pool_bwd(d, X, d_out, argmax, bind.rows_args(None, seen, rowbase, touched, touched_count, marks),
                                 status))


def scatter_pool_bwd_det(grad_tables, X, singles, pooled, d_out, acc64, marks, argmax=None, amax_slot=None,
                         clear_marks=True, status=None, amax_supplied=False, defer_totals=False, flags=None):
    """Deterministic form of scatter_pool_bwd (mml_scatter_pool_bwd_det): acc64 = one int64 [V, E] accumulator per TABLE
    (all zero between calls), marks = the byte map of marks_bytes(table sizes).  Bitwise repeatable, independent of the
    order of the samples; tables shared by several fields are allowed.  amax_supplied / defer_totals as in
    scatter_bwd_det, with scatter_pool_det_shift(...) as the totals' shift.  `flags` (an int) replaces the three switches."""
    _need_gpu(X, d_out)
    d = make_pool_desc(grad_tables, singles, pooled)
    if amax_slot is None:
        amax_slot = amax_slots(1, X.device)[0]
    if flags is None:
        flags = ((L.SCATTER_DET_CLEAR_MARKS if clear_marks else 0) | (L.SCATTER_DET_AMAX_SUPPLIED if amax_supplied else 0) |
                 (L.SCATTER_DET_DEFER_TOTALS if defer_totals else 0))
    _issue(bind.scatter_pool_bwd_det(d, X, d_out, argmax, acc64, amax_slot, marks, flags, status))


def scatter_pool_det_shift(desc, B):
    """log2 of the fixed-point scale the deterministic pooled scatter uses for B samples (mml_scatter_pool_det_shift):
    `desc` = a PoolDesc (make_pool_desc) or (table sizes, E, singles, pooled).  Negative: B times the lookups of one
    table leave no headroom in the 64-bit totals (the scatter refuses such a batch)."""
    if not isinstance(desc, L.PoolDesc):
        vocab, E, singles, pooled = desc
        desc = make_pool_desc(None, singles, pooled, vocab=(list(vocab), E))
    return int(L.load().mml_scatter_pool_det_shift(C.byref(desc), int(B)))


def index_unique_pool(vocab, E, X, singles, pooled, seen, rowbase, touched, touched_count, status=None, marks=None):
    """The distinct VALID rows of a batch per table, without gradients (mml_index_unique_pool)."""
    _need_gpu(X, touched, touched_count)
    d = make_pool_desc(None, singles, pooled, vocab=(list(vocab), E))
    _issue(bind.index_unique_pool(d, X, bind.rows_args(None, seen, rowbase, touched, touched_count, marks), status))


def marks_bytes(vocab):
    """Size of the row-mark scratch map of mml_scatter_bwd / mml_index_unique (include/mmlrec.h: row_marks); the layout
    is defined once in C: mark_bases (csrc/scatter_fold.hpp)."""
    return 32 * sum((int(v) + 31) // 32 for v in vocab)


def scatter_bwd(grad_tables, X, cols, d_out, seen=None, rowbase=None, touched=None, touched_count=None, status=None,
                marks=None):
    """grad_tables[f][X[:, cols[f]].long()] += d_out[:, f*E:(f+1)*E] (float atomics)."""
    _need_gpu(X, d_out, *grad_tables)
    _issue(bind.scatter_bwd(grad_tables, X, cols, d_out,
                            bind.rows_args(None, seen, rowbase, touched, touched_count, marks), status))


def scatter_bwd_det(grad_tables, X, cols, d_out, acc64, marks, amax_slot=None, clear_marks=True, status=None,
                    amax_supplied=False, defer_totals=False):
    """Deterministic scatter (mml_scatter_bwd_det): acc64 = per-table int64 [V, E] accumulators (all zero between calls),
    marks = the byte map of marks_bytes(vocab).  Bitwise repeatable, independent of the order of the samples.
    amax_supplied: amax_slot already holds the magnitude of d_out (no magnitude pass); defer_totals: the totals stay in
    acc64 and the marks set, for opt_step_dense entries that carry (acc64, slot, scatter_det_shift(B))."""
    _need_gpu(X, d_out, *grad_tables)
    if amax_slot is None:
        amax_slot = amax_slots(1, X.device)[0]
    flags = ((L.SCATTER_DET_CLEAR_MARKS if clear_marks else 0) | (L.SCATTER_DET_AMAX_SUPPLIED if amax_supplied else 0) |
             (L.SCATTER_DET_DEFER_TOTALS if defer_totals else 0))
    _issue(bind.scatter_bwd_det(grad_tables, X, cols, d_out, acc64, amax_slot, marks, flags, status))


def scatter_det_shift(B):
    """log2 of the fixed-point scale the deterministic scatter uses for B samples (mml_opt_tensor.acc_shift)."""
    return int(L.load().mml_scatter_det_shift(int(B)))


def scatter_bwd_idx32(grad_tables, idx, d_out, seen=None, rowbase=None, touched=None, touched_count=None, status=None,
                      marks=None):
    """grad_tables[f][idx[:, f]] += d_out[:, f*E:(f+1)*E] with native int32 indices [B, F]."""
    _need_gpu(idx, d_out, *grad_tables)
    _issue(bind.scatter_bwd_idx32(grad_tables, idx, d_out,
                                  bind.rows_args(None, seen, rowbase, touched, touched_count, marks), status))


def route(X, cols, vocab, keybase, world, status=None):
    """Row-sharded routing of a batch (csrc/shard.hip): returns (counts [world] int32, send_keys [B*F] int32 grouped by
    owner, pos [B, F] int32)."""
    lib = L.load()
    _need_gpu(X)
    F, B = len(vocab), X.shape[0]
    col = (L.i32 * F)(*cols)
    voc = (L.i64 * F)(*vocab)
    kb = (L.i64 * F)(*keybase[:F])
    counters = torch.zeros(2 * world, dtype=torch.int32, device=X.device)
    keys = torch.empty(B * F, dtype=torch.int32, device=X.device)
    pos = torch.empty(B, F, dtype=torch.int32, device=X.device)
    s = _stream()
    if X.dtype == torch.int32:
        xa = (None, 0, X.data_ptr(), X.stride(0))
    else:
        xa = (_f32_2d(X, "X").data_ptr(), _ld(X), None, 0)
    L.check(lib.mml_route_count(*xa, col, voc, F, B, world, counters.data_ptr(), L.ptr(status), s), "mml_route_count")
    counts = counters[:world].clone()
    L.check(lib.mml_route_place(*xa, col, voc, kb, F, B, world, counters.data_ptr(), keys.data_ptr(), pos.data_ptr(),
                                L.ptr(status), s), "mml_route_place")
    return counts, keys, pos


def rows_permute(src, pos, E, dst):
    """dst[pos[b, f]] = src[b, f*E:(f+1)*E]."""
    B, F = pos.shape
    L.check(L.load().mml_rows_permute(src.data_ptr(), _ld(src), pos.data_ptr(), F, E, B, dst.data_ptr(), _stream()),
            "mml_rows_permute")


# ---------------------------------------------------------------------------------------------- K3
def make_fwd_descs(problems):
    """problems: dicts with A [M,K], W ([N,K] or [K,N] if w_kn), bias or None, C [M,N], act, w_kn."""
    arr = (L.GemmFwdDesc * len(problems))()
    for d, p in zip(arr, problems):
        A, W, Cc = p["A"], p["W"], p["C"]
        w_kn = int(p.get("w_kn", 0))
        d.A, d.W, d.C = A.data_ptr(), W.data_ptr(), Cc.data_ptr()
        d.bias = L.ptr(p.get("bias"))
        d.lda, d.ldw, d.ldc = _ld(A), _ld(W), _ld(Cc)
        d.M, d.K = A.shape
        d.N = W.shape[1] if w_kn else W.shape[0]
        d.act = int(p.get("act", L.ACT_NONE))
        d.w_kn = w_kn
        m = p.get("mask")
        d.relu_mask = L.ptr(m)
        d.ldmask = _ld(m) if m is not None else 0
        d.amax_a, d.amax_w, d.amax_out = L.ptr(p.get("amax_a")), L.ptr(p.get("amax_w")), L.ptr(p.get("amax_out"))
        d.w_planes, d.w_kexp = L.ptr(p.get("w_planes")), L.ptr(p.get("w_kexp"))  # pre-cut weight (planes_cut)
        mul, prod = p.get("mul"), p.get("prod")  # K7: prod = C * mul from the same epilogue
        if mul is not None:
            d.mul, d.prod, d.ldmul, d.ldprod = mul.data_ptr(), prod.data_ptr(), _ld(mul), _ld(prod)
            d.amax_prod = L.ptr(p.get("amax_prod"))
    return arr


# ---- operand magnitudes (include/mmlrec.h): slots of MML_AMAX_WORDS words --------------------------------------
AMAX_WORDS = 8
PLANES_ROWS, PLANES_COLS = 0, 1


def make_planes_descs(items):
    """items: (W [rows, cols] view, planes int32 tensor of W's shape and pitch, layout, [magnitude slots], kexp int32
    [1] tensor) -> the descriptor block of mml_gemm_planes_cut."""
    arr = (L.PlanesDesc * len(items))()
    for d, (W, planes, layout, slots, kexp) in zip(arr, items):
        # K6: W = (A, B) -> the planes of the element-wise product A * B; slots = [(slot of A_i, slot of B_i)] for the
        # matrices of the group that shares the exponent
        W2 = None
        if isinstance(W, tuple):
            W, W2 = W
            if W2.shape != W.shape:
                raise L.MMLError("factors of a derived weight must have one shape")
            if 2 * len(slots) > L.MAX_SRC:
                raise L.MMLError("too many product weights share one exponent")
        # planes: the weight's shape (pitch may differ), or -- for the zero-padded operand of a reduction that is not a
        # multiple of 16 -- the same rows with the columns rounded up (a zero-initialised buffer)
        if planes.shape[0] != W.shape[0] or planes.shape[1] < W.shape[1]:
            raise L.MMLError("planes buffer must have the weight's rows and at least its columns")
        d.W, d.planes = W.data_ptr(), planes.data_ptr()
        d.rows, d.cols = W.shape
        d.ld = _ld(W)
        d.ldp = _ld(planes)
        d.layout = int(layout)
        d.n_amax = len(slots)
        if W2 is not None:
            d.W2, d.ld2 = W2.data_ptr(), _ld(W2)
            for a, (sa, sb) in enumerate(slots):
                d.amax[a] = sa.data_ptr()
                d.amax[len(slots) + a] = sb.data_ptr()
        else:
            for a, sl in enumerate(slots):
                d.amax[a] = sl.data_ptr()
        d.kexp = kexp.data_ptr()
    return arr


def planes_cut(items):
    """Cut weight matrices into their two fp16 planes once (include/mmlrec.h: mml_gemm_planes_cut)."""
    arr = make_planes_descs(items)
    L.check(L.load().mml_gemm_planes_cut(arr, len(items), _stream()), "mml_gemm_planes_cut")


def amax_slots(n, device):
    """n zeroed magnitude slots as an int32 [n, AMAX_WORDS] tensor (row i = slot i)."""
    return torch.zeros(n, AMAX_WORDS, dtype=torch.int32, device=device)


def make_amax_descs(pairs):
    """pairs: (tensor [rows, cols] with unit column stride, slot) -- one mml_amax_batch call raises every slot."""
    arr = (L.AmaxDesc * len(pairs))()
    for d, (x, slot) in zip(arr, pairs):
        if x.dim() == 1:
            x = x.view(1, -1)
        d.x, d.rows, d.cols, d.ld, d.slot = x.data_ptr(), x.shape[0], x.shape[1], _ld(x), slot.data_ptr()
    return arr


def amax_batch(pairs):
    arr = make_amax_descs(pairs)
    L.check(L.load().mml_amax_batch(arr, len(pairs), _stream()), "mml_amax_batch")


def amax_value(slot):
    """The slot's value as a Python float (host read: tests / diagnostics)."""
    return float(slot.view(-1).max().view(1).view(torch.float32).item())


def _measured(tensors, cache):
    """slot per tensor (by storage pointer + shape), measured now with the stand-alone kernel"""
    todo = []
    for t in tensors:
        key = (t.data_ptr(), tuple(t.shape), t.stride(0) if t.dim() > 1 else 0)
        if key not in cache:
            cache[key] = amax_slots(1, t.device)[0]
            todo.append((t, cache[key]))
    if todo:
        amax_batch(todo)
    return cache


def gemm_fwd(problems, amax=False):
    """amax=True: measure both operands of every problem first (stand-alone mml_amax_batch launches), which lets the
    launch run the two-plane fp16 arithmetic -- what engine.py arranges with magnitudes produced along the way."""
    lib = L.load()
    if amax:
        cache = _measured([p["A"] for p in problems] + [p["W"] for p in problems], {})
        problems = [dict(p, amax_a=cache[(p["A"].data_ptr(), tuple(p["A"].shape), p["A"].stride(0))],
                         amax_w=cache[(p["W"].data_ptr(), tuple(p["W"].shape), p["W"].stride(0))]) for p in problems]
    arr = make_fwd_descs(problems)
    L.check(lib.mml_gemm_grouped_fwd(arr, len(problems), _stream()), "mml_gemm_grouped_fwd")


def make_dgrad_descs(problems):
    """problems: dicts with dA [M,K], Y (or None), act, accumulate, srcs = [(dC [M,N], W, w_kn), ...]."""
    arr = (L.GemmDgradDesc * len(problems))()
    for d, p in zip(arr, problems):
        gate = p.get("gate")  # K7 backward: dict(h, g, dh, dg, act_h, act_g, acc_h, acc_g[, amax_dh, amax_dg]); no dA
        if gate is not None:
            d.gate_h, d.gate_g, d.d_h, d.d_g = (gate[k].data_ptr() for k in ("h", "g", "dh", "dg"))
            d.ld_h, d.ld_g, d.ld_dh, d.ld_dg = (_ld(gate[k]) for k in ("h", "g", "dh", "dg"))
            d.act_h, d.act_g, d.acc_h, d.acc_g = (int(gate[k]) for k in ("act_h", "act_g", "acc_h", "acc_g"))
            d.amax_dh, d.amax_dg = L.ptr(gate.get("amax_dh")), L.ptr(gate.get("amax_dg"))
        dA = p["dA"] if gate is None else gate["dh"]
        d.dA = dA.data_ptr() if gate is None else None
        Y = p.get("Y")
        d.Y = L.ptr(Y)
        d.ldda = _ld(dA)
        d.ldy = _ld(Y) if Y is not None else 0
        d.M, d.K = dA.shape
        d.act = int(p.get("act", L.ACT_NONE)) if Y is not None else L.ACT_NONE
        d.accumulate = int(p.get("accumulate", 0))
        srcs = p["srcs"]
        d.n_src = len(srcs)
        for s, src in enumerate(srcs):
            dC, W, w_kn = src[:3]
            d.dC[s], d.W[s] = dC.data_ptr(), W.data_ptr()
            d.lddc[s], d.ldw[s] = _ld(dC), _ld(W)
            d.N[s] = dC.shape[1]
            d.w_kn[s] = int(w_kn)
            if len(src) > 3:  # (dC, W, w_kn, magnitude slot of dC, magnitude slot of W[, planes of W, their exponent])
                d.amax_dc[s], d.amax_w[s] = L.ptr(src[3]), L.ptr(src[4])
            if len(src) > 5:
                d.w_planes[s], d.w_kexp[s] = L.ptr(src[5]), L.ptr(src[6])
        m = p.get("mask")
        d.relu_mask = L.ptr(m)
        d.ldmask = _ld(m) if m is not None else 0
        d.amax_out = L.ptr(p.get("amax_out"))
    return arr


def gemm_dgrad(problems, amax=False):
    lib = L.load()
    if amax:
        ts = [t for p in problems for src in p["srcs"] for t in src[:2]]
        cache = _measured(ts, {})
        k = lambda t: (t.data_ptr(), tuple(t.shape), t.stride(0))  # noqa: E731
        problems = [dict(p, srcs=[(dC, W, kn, cache[k(dC)], cache[k(W)]) for dC, W, kn in
                                  [src[:3] for src in p["srcs"]]]) for p in problems]
    arr = make_dgrad_descs(problems)
    L.check(lib.mml_gemm_grouped_dgrad(arr, len(problems), _stream()), "mml_gemm_grouped_dgrad")


def make_wgrad_descs(problems):
    """problems: dicts with dC [M,N], A [M,K], dW ([N,K] or [K,N] if w_kn), dbias or None, accumulate, w_kn."""
    arr = (L.GemmWgradDesc * len(problems))()
    for d, p in zip(arr, problems):
        dC, A, dW = p["dC"], p["A"], p["dW"]
        d.dC, d.A, d.dW = dC.data_ptr(), A.data_ptr(), dW.data_ptr()
        d.dbias = L.ptr(p.get("dbias"))
        d.lddc, d.lda, d.lddw = _ld(dC), _ld(A), _ld(dW)
        d.M, d.N = dC.shape
        d.K = A.shape[1]
        d.accumulate = int(p.get("accumulate", 0))
        d.w_kn = int(p.get("w_kn", 0))
        d.amax_dc, d.amax_a = L.ptr(p.get("amax_dc")), L.ptr(p.get("amax_a"))
    return arr


def gemm_wgrad(problems, amax=False):
    lib = L.load()
    if amax:
        cache = _measured([p["dC"] for p in problems] + [p["A"] for p in problems], {})
        k = lambda t: (t.data_ptr(), tuple(t.shape), t.stride(0))  # noqa: E731
        problems = [dict(p, amax_dc=cache[k(p["dC"])], amax_a=cache[k(p["A"])]) for p in problems]
    arr = make_wgrad_descs(problems)
    dev = problems[0]["dC"].device
    nbytes = lib.mml_gemm_grouped_wgrad_workspace_bytes(arr, len(problems))
    ws = workspace(nbytes, dev)
    L.check(lib.mml_gemm_grouped_wgrad(arr, len(problems), ws.data_ptr(), ws.numel(), _stream()),
            "mml_gemm_grouped_wgrad")


# ---------------------------------------------------------------------------------------------- K4
def make_gate_group(experts, gates, B, H, d_experts=None, e_relu=True):
    """experts: list of [B,H] tensors; gates: dicts with G, Wg, P, mix, expert (index list) and, for backward,
    dmix, dG, dWg, g_relu, active."""
    g = L.GateGroup()
    g.n_experts, g.n_gates, g.H, g.B, g.e_relu = len(experts), len(gates), H, B, int(e_relu)
    for x, e in enumerate(experts):
        g.E[x], g.lde[x] = e.data_ptr(), _ld(e)
        if d_experts is not None:
            g.dE[x], g.ldde[x] = d_experts[x].data_ptr(), _ld(d_experts[x])
    for i, q in enumerate(gates):
        d = g.gate[i]
        G, Wg, P = q["G"], q["Wg"], q["P"]
        d.G, d.Wg, d.P = G.data_ptr(), Wg.data_ptr(), P.data_ptr()
        d.ldg, d.ldp = _ld(G), _ld(P)
        d.ne, d.Gd = Wg.shape
        if not Wg.is_contiguous():
            raise L.MMLError("gate weight must be contiguous")
        if q.get("mix") is not None:
            d.mix, d.ldmix = q["mix"].data_ptr(), _ld(q["mix"])
        d.active = int(q.get("active", 1))
        d.g_relu = int(q.get("g_relu", 1))
        if q.get("dmix") is not None:
            d.dmix, d.lddmix = q["dmix"].data_ptr(), _ld(q["dmix"])
        if q.get("dG") is not None:
            d.dG, d.lddg = q["dG"].data_ptr(), _ld(q["dG"])
        if q.get("dWg") is not None:
            d.dWg = q["dWg"].data_ptr()
        for s, x in enumerate(q["expert"]):
            d.expert[s] = x
    # bf16-storage path: tensors only GEMMs read may be bf16 buffers (include/mmlrec.h: mml_gate_group.out_bf16)
    def _all16(ts, what):
        ts = [t for t in ts if t is not None]
        n16 = sum(t.dtype == torch.bfloat16 for t in ts)
        if n16 not in (0, len(ts)):
            raise L.MMLError(f"gate group: {what} must be all bf16 or all fp32")
        return bool(ts) and n16 == len(ts)
    bits = 0
    if _all16([q.get("mix") for q in gates], "mix"):
        bits |= L.GATE_MIX_BF16
    if d_experts is not None and _all16(list(d_experts), "dE"):
        bits |= L.GATE_DE_BF16
    if _all16([q.get("dG") for q in gates], "dG"):
        bits |= L.GATE_DG_BF16
    if _all16(list(experts), "E"):
        bits |= L.GATE_E_BF16
    g.out_bf16 = bits
    return g


def gate_mix_fwd(group):
    lib = L.load()
    L.check(lib.mml_gate_mix_fwd(C.byref(group), _stream()), "mml_gate_mix_fwd")


def gate_mix_bwd(group, device, phases=False):
    """phases: the two-launch form (row kernel, then the reduction of its partial sums)."""
    lib = L.load()
    ws = workspace(lib.mml_gate_mix_bwd_workspace_bytes(C.byref(group)), device)
    if phases:
        for ph in (1, 2):
            L.check(lib.mml_gate_mix_bwd_phase(C.byref(group), ws.data_ptr(), ws.numel(), ph, _stream()),
                    "mml_gate_mix_bwd_phase")
        return
    L.check(lib.mml_gate_mix_bwd(C.byref(group), ws.data_ptr(), ws.numel(), _stream()), "mml_gate_mix_bwd")


# ---------------------------------------------------------------------------------------------- K5
def make_head_group(heads, prob, y=None, mask=None, loss=None, dprob=None):
    """heads: dicts with Hin [B,H], w [H] (any shape with H elements), bias [1], optional w2, bias2 (list of 1-element
    tensors packed by the caller into one tensor), dH, dw, dbias, h_relu, mask_col, kind (L.head_kind(out, loss); default 0 =
    sigmoid + BCE); gated heads also gate [B,H], dgate, gate_act."""
    g = L.HeadGroup()
    g.n_heads = len(heads)
    g.B = prob.shape[0]
    g.prob, g.ldprob = prob.data_ptr(), _ld(prob)
    if y is not None:
        g.y, g.ldy = y.data_ptr(), _ld(y)
    if mask is not None:
        g.mask, g.ldmask = mask.data_ptr(), _ld(mask)
    g.loss = L.ptr(loss)
    if dprob is not None:
        g.dprob, g.lddprob = dprob.data_ptr(), _ld(dprob)
    for t, q in enumerate(heads):
        d = g.head[t]
        Hin = q["Hin"]
        d.Hin, d.ldh, d.H = Hin.data_ptr(), _ld(Hin), Hin.shape[1]
        d.w, d.bias = q["w"].data_ptr(), q["bias"].data_ptr()
        d.w2 = L.ptr(q.get("w2"))
        b2 = q.get("bias2")
        d.bias2 = L.ptr(b2)
        d.n_bias2 = 0 if b2 is None else b2.numel()
        if q.get("dH") is not None:
            d.dH, d.lddh = q["dH"].data_ptr(), _ld(q["dH"])
        d.dw, d.dbias = L.ptr(q.get("dw")), L.ptr(q.get("dbias"))
        d.h_relu = int(q.get("h_relu", 1))
        d.mask_col = int(q.get("mask_col", -1))
        d.kind = int(q.get("kind", 0))
        if q.get("gate") is not None:  # gated head: the input is Hin (.) gate (include/mmlrec.h: mml_head_desc.gate)
            d.gate, d.ldgate = q["gate"].data_ptr(), _ld(q["gate"])
            d.gate_act = int(q.get("gate_act", L.ACT_NONE))
            if q.get("dgate") is not None:
                d.dgate, d.lddgate = q["dgate"].data_ptr(), _ld(q["dgate"])
    dhs = [q["dH"] for q in heads if q.get("dH") is not None]
    n16 = sum(t.dtype == torch.bfloat16 for t in dhs)
    if n16 not in (0, len(dhs)):
        raise L.MMLError("head group: dH must be all bf16 or all fp32")
    g.dh_bf16 = int(bool(dhs) and n16 == len(dhs))  # (include/mmlrec.h: mml_head_group.dh_bf16)
    return g


def make_tower_head_group(tasks, prob, y, mask=None, loss=None):
    """K5' (include/mmlrec.h): tasks = dicts with A [M, K], amax_a, planes_fwd / kexp_fwd (MML_PLANES_ROWS image of the tower
    weight [N, K]), planes_bwd / kexp_bwd (MML_PLANES_COLS), bias1 [N] or None, w [N], hbias [1], hbias2 or None, dH [M, N],
    dA [M, K], dw [N], dhbias [1], optional amax_dH / amax_dA, mask_col, head (column of prob / y), kind (as in make_head_group)."""
    g = L.TowerHeadGroup()
    g.n, g.M = len(tasks), prob.shape[0]
    g.prob, g.ldprob = prob.data_ptr(), _ld(prob)
    g.y, g.ldy = y.data_ptr(), _ld(y)
    if mask is not None:
        g.mask, g.ldmask = mask.data_ptr(), _ld(mask)
    g.loss = L.ptr(loss)
    for t, q in enumerate(tasks):
        d = g.t[t]
        A = q["A"]
        d.A, d.lda, d.K = A.data_ptr(), _ld(A), A.shape[1]
        d.N = q["dH"].shape[1]
        d.amax_a = q["amax_a"].data_ptr()
        d.w_planes_fwd, d.ldpf, d.kexp_fwd = q["planes_fwd"].data_ptr(), _ld(q["planes_fwd"]), q["kexp_fwd"].data_ptr()
        d.w_planes_bwd, d.ldpb, d.kexp_bwd = q["planes_bwd"].data_ptr(), _ld(q["planes_bwd"]), q["kexp_bwd"].data_ptr()
        d.bias1 = L.ptr(q.get("bias1"))
        d.w, d.hbias = q["w"].data_ptr(), q["hbias"].data_ptr()
        b2 = q.get("hbias2")
        d.hbias2, d.n_hbias2 = L.ptr(b2), (0 if b2 is None else b2.numel())
        d.dH, d.lddh = q["dH"].data_ptr(), _ld(q["dH"])
        d.dA, d.ldda = q["dA"].data_ptr(), _ld(q["dA"])
        d.dw, d.dhbias = q["dw"].data_ptr(), q["dhbias"].data_ptr()
        d.amax_dH, d.amax_dA = L.ptr(q.get("amax_dH")), L.ptr(q.get("amax_dA"))
        d.mask_col, d.head = int(q.get("mask_col", -1)), int(q.get("head", t))
        d.kind = int(q.get("kind", 0))
    return g


def tower_head_fwd_bwd(group, device, phases=False):
    lib = L.load()
    n = int(lib.mml_tower_head_workspace_bytes(C.byref(group)))
    if n < 0:
        L.check(-1, "mml_tower_head_workspace_bytes")
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device=device)
    for ph in ((1, 2) if phases else (0,)):
        L.check(lib.mml_tower_head_fwd_bwd(C.byref(group), ws.data_ptr(), ws.numel(), ph, _stream()), "mml_tower_head_fwd_bwd")
    return ws


def head_fwd(group):
    lib = L.load()
    L.check(lib.mml_head_fwd(C.byref(group), _stream()), "mml_head_fwd")


def head_bce_fwd_bwd(group, device, phases=False):
    lib = L.load()
    ws = workspace(lib.mml_head_workspace_bytes(C.byref(group)), device)
    if phases:
        for ph in (1, 2):
            L.check(lib.mml_head_bce_fwd_bwd_phase(C.byref(group), ws.data_ptr(), ws.numel(), ph, _stream()),
                    "mml_head_bce_fwd_bwd_phase")
        return
    L.check(lib.mml_head_bce_fwd_bwd(C.byref(group), ws.data_ptr(), ws.numel(), _stream()), "mml_head_bce_fwd_bwd")


def rows_phase1_then_batched_reduce(head_groups, gate_groups, device):
    """The row kernels of the given head / gate groups (phase 1, each into a workspace of its own), then ALL their
    reductions in one launch (include/mmlrec.h: mml_rows_reduce_batch)."""
    lib = L.load()
    items = (L.RowsReduceItem * (len(head_groups) + len(gate_groups)))()
    keep, k = [], 0
    for kind, groups in ((L.ROWS_REDUCE_HEAD, head_groups), (L.ROWS_REDUCE_GATE, gate_groups)):
        for g in groups:
            if kind == L.ROWS_REDUCE_HEAD:
                ws = torch.empty(max(int(lib.mml_head_workspace_bytes(C.byref(g))), 256), dtype=torch.uint8, device=device)
                L.check(lib.mml_head_bce_fwd_bwd_phase(C.byref(g), ws.data_ptr(), ws.numel(), 1, _stream()),
                        "mml_head_bce_fwd_bwd_phase")
            else:
                ws = torch.empty(max(int(lib.mml_gate_mix_bwd_workspace_bytes(C.byref(g))), 256), dtype=torch.uint8,
                                 device=device)
                L.check(lib.mml_gate_mix_bwd_phase(C.byref(g), ws.data_ptr(), ws.numel(), 1, _stream()),
                        "mml_gate_mix_bwd_phase")
            keep.append(ws)
            items[k].kind, items[k].group = kind, C.addressof(g)
            items[k].workspace, items[k].workspace_bytes = ws.data_ptr(), ws.numel()
            k += 1
    L.check(lib.mml_rows_reduce_batch(items, k, _stream()), "mml_rows_reduce_batch")
    return keep


# ---------------------------------------------------------------------------------------------- K6/K7
def ew_mul(a, b, out):
    _issue(bind.ew_mul(a, b, out))


def ew_mul_bwd(dout, a, b, da=None, db=None, acc_a=False, acc_b=False):
    _issue(bind.ew_mul_bwd(dout, a, b, da, db, acc_a, acc_b))


def ew_add_n(inputs, out):
    _issue(bind.ew_add_n(inputs, out))


def dropout(x, out, p, seed, site=0, step=0, step_dev=None, accumulate=False, row0=0):
    """out (+)= x * keep / (1 - p) on [rows, cols] views (row pitches may differ; out may be x); the backward is the same
    call on the gradient (include/mmlrec.h: mml_dropout; reference model/utils.py:159)."""
    _issue(bind.dropout(x, out, p, seed, site, step_dev, step, accumulate, row0))


def copy2d(src, dst, accumulate=False):
    """dst[:, :] (+)= src[:, :] for 2-D row-strided views (column slices of wider buffers are fine)."""
    _issue(bind.copy2d(src, dst, accumulate))


def make_sumprod_descs(rows, too_many="more than 8 terms in one sum"):
    """The SumProdDesc block of mml_sumprod_batch: out (+)= sum_k x_k * (y_k or 1) over n flat elements per row.
    rows: (out, n, [(x, y or None), ...], accumulate, act, deriv_of[, amax slot]) -- act != ACT_NONE multiplies the sum by
    act'(deriv_of); the slot is raised with the magnitude of what is stored.  too_many: the caller's words for a row of
    more than 8 terms."""
    arr = (L.SumProdDesc * len(rows))()
    for d, row in zip(arr, rows):
        out, n, terms, acc, act, deriv_of = row[:6]
        if len(terms) > 8:
            raise NotImplementedError(too_many)
        d.out, d.n, d.n_terms, d.accumulate = out.data_ptr(), n, len(terms), int(acc)
        d.amax_out = L.ptr(row[6]) if len(row) > 6 else None
        d.act, d.deriv_of = int(act), (deriv_of.data_ptr() if act != L.ACT_NONE else None)
        for k, (x, y) in enumerate(terms):
            d.x[k], d.y[k] = x.data_ptr(), L.ptr(y)
    return arr


def make_attn2_desc(tokens, out, A, B, H, sqrt_h, grads=None):
    """mml_attn2_desc: tokens = [(V, K, Q)] x 2 of [B, H] views, out [B, H], A = the [B, 2] attention weights the forward
    leaves for the backward; grads = (dout, [(dV, dK, dQ)] x 2) for mml_attn2_bwd."""
    d = L.Attn2Desc()
    for t, (V, K, Q) in enumerate(tokens):
        d.V[t], d.K[t], d.Q[t] = V.data_ptr(), K.data_ptr(), Q.data_ptr()
        d.ldv[t], d.ldk[t], d.ldq[t] = _ld(V), _ld(K), _ld(Q)
    d.out, d.ldo, d.A = out.data_ptr(), _ld(out), A.data_ptr()
    d.B, d.H, d.sqrt_h = B, H, sqrt_h
    if grads is not None:
        dout, dtokens = grads
        d.dout, d.lddo = dout.data_ptr(), _ld(dout)
        for t, (dV, dK, dQ) in enumerate(dtokens):
            d.dV[t], d.dK[t], d.dQ[t] = dV.data_ptr(), dK.data_ptr(), dQ.data_ptr()
            d.lddv[t], d.lddk[t], d.lddq[t] = _ld(dV), _ld(dK), _ld(dQ)
    return d


def prelu_max_batch():
    return int(L.load().mml_prelu_max_batch())


def make_prelu_descs(items):
    """items: dicts z, y [rows, cols] views, alpha (a device tensor holding the slope), optional amax (a slot)."""
    arr = (L.PreluDesc * len(items))()
    for d, it in zip(arr, items):
        z, y = _f32_2d(it["z"], "prelu z"), _f32_2d(it["y"], "prelu y")
        if y.shape != z.shape or it["alpha"].dtype != torch.float32 or it["alpha"].numel() != 1:
            raise L.MMLError("prelu: y must have z's shape and alpha one float32 element")
        d.z, d.ldz, d.y, d.ldy, d.rows, d.cols = z.data_ptr(), _ld(z), y.data_ptr(), _ld(y), z.shape[0], z.shape[1]
        d.alpha, d.amax_out = it["alpha"].data_ptr(), L.ptr(it.get("amax"))
    return arr


def make_prelu_bwd_descs(items, seen=None):
    """items: dicts dy, z, dz [rows, cols] views (dz may be dy), alpha, dalpha (one-element device tensors), optional
    acc_dz, acc_dalpha, amax.  seen: the dalpha addresses earlier launches of the same backward already wrote -- an item
    that names one of them accumulates."""
    arr = (L.PreluBwdDesc * len(items))()
    for d, it in zip(arr, items):
        dy, z, dz = _f32_2d(it["dy"], "prelu dy"), _f32_2d(it["z"], "prelu z"), _f32_2d(it["dz"], "prelu dz")
        if dy.shape != z.shape or dz.shape != z.shape:
            raise L.MMLError("prelu backward: dy, z and dz must have one shape")
        for k in ("alpha", "dalpha"):
            if it[k].dtype != torch.float32 or it[k].numel() != 1:
                raise L.MMLError(f"prelu backward: {k} must be one float32 element")
        d.dy, d.lddy, d.z, d.ldz, d.dz, d.lddz = dy.data_ptr(), _ld(dy), z.data_ptr(), _ld(z), dz.data_ptr(), _ld(dz)
        d.rows, d.cols, d.alpha, d.dalpha = z.shape[0], z.shape[1], it["alpha"].data_ptr(), it["dalpha"].data_ptr()
        d.accumulate_dz = int(bool(it.get("acc_dz")))
        d.accumulate_dalpha = int(bool(it.get("acc_dalpha")) or (seen is not None and d.dalpha in seen))
        d.amax_out = L.ptr(it.get("amax"))
    return arr


def prelu_chunks(items):
    """A list of problems in launches of at most mml_prelu_max_batch() items."""
    cap = prelu_max_batch()
    return [items[i:i + cap] for i in range(0, len(items), cap)]


def prelu_fwd(items):
    """y = z > 0 ? z : alpha * z for a list of problems, ONE launch per mml_prelu_max_batch() of them."""
    _need_gpu(*[it["z"] for it in items])
    for chunk in prelu_chunks(items):
        L.check(L.load().mml_prelu_batch_fwd(make_prelu_descs(chunk), len(chunk), _stream()), "mml_prelu_batch_fwd")


def prelu_bwd(items):
    """dz (+)= z > 0 ? dy : alpha * dy and dalpha (+)= sum_{z <= 0} dy * z; items that share a dalpha tensor are summed
    into it (include/mmlrec.h: mml_prelu_batch_bwd)."""
    _need_gpu(*[it["z"] for it in items])
    seen = set()
    for chunk in prelu_chunks(items):
        arr = make_prelu_bwd_descs(chunk, seen)
        # an item whose dalpha an EARLIER item of this launch names must carry that item's flag
        first = {}
        for d in arr:
            d.accumulate_dalpha = first.setdefault(d.dalpha, d.accumulate_dalpha)
        nbytes = int(L.load().mml_prelu_workspace_bytes(len(chunk)))
        ws = workspace(nbytes, chunk[0]["z"].device)
        L.check(L.load().mml_prelu_batch_bwd(arr, len(chunk), ws.data_ptr(), nbytes, _stream()), "mml_prelu_batch_bwd")
        seen.update(d.dalpha for d in arr)


def make_pcgrad_segs(segs, T, need_out=False):
    """segs: dicts `banks` (T entries: objective t's gradient of one parameter tensor -- float32, 1-D or 2-D with unit
    inner stride, one shape and row pitch for all -- or None = no gradient), optional `out` (same layout; may be one of
    the banks) and `marks` (uint8, one byte per row).  Returns the mml_pcgrad_seg array (include/mmlrec.h)."""
    arr = (L.PcgradSeg * max(len(segs), 1))()
    for d, sg in zip(arr, segs):
        banks = list(sg["banks"])
        if len(banks) != T:
            raise L.MMLError(f"pcgrad: a segment has {len(banks)} banks for T = {T}")
        have = [b for b in banks if b is not None] + ([sg["out"]] if sg.get("out") is not None else [])
        if not have:
            raise L.MMLError("pcgrad: a segment whose banks are all None")
        _need_gpu(*have)
        ref = have[0]
        for b in have:
            if (b.dtype != torch.float32 or b.dim() not in (1, 2) or b.shape != ref.shape or b.stride() != ref.stride() or
                    (b.shape[-1] > 1 and b.stride(-1) != 1)):
                raise L.MMLError("pcgrad: banks and out of a segment must be float32 views of one shape and pitch")
        rows, cols = (1, ref.shape[0]) if ref.dim() == 1 else ref.shape
        for k, b in enumerate(banks):
            d.bank[k] = b.data_ptr() if b is not None else None
        d.out = L.ptr(sg.get("out"))
        d.rows, d.cols, d.ld = rows, cols, (cols if ref.dim() == 1 else _ld(ref))
        marks = sg.get("marks")
        if marks is not None and (marks.dtype != torch.uint8 or marks.numel() < rows or not marks.is_contiguous()):
            raise L.MMLError("pcgrad: marks must be a contiguous uint8 tensor with one byte per row")
        d.row_marks = L.ptr(marks)
        if need_out and sg.get("out") is None:
            raise L.MMLError("pcgrad combine: a segment without `out`")
    return arr


def pcgrad_gram(segs, T, gram=None):
    """The T x T Gram matrix (float64, device) of the per-objective gradients over every segment: one pass, fixed-order
    sums (mml_pcgrad_gram)."""
    arr = make_pcgrad_segs(segs, T)
    dev = next(b for b in segs[0]["banks"] if b is not None).device
    if gram is None:
        gram = torch.empty((T, T), dtype=torch.float64, device=dev)
    nbytes = int(L.load().mml_pcgrad_workspace_bytes(arr, len(segs), T))
    _issue(bind.pcgrad_gram(arr, len(segs), T, gram, workspace(nbytes, dev)))  # (the byte count is only checked)
    return gram


def pcgrad_weights(gram, order, w=None, fired=None):
    """gram [T, T] float64, order [T, T] int32 (row i: the order in which g_i meets the g_j), both on the device ->
    (w [2 T] float32: mean weights then sum weights, fired [T, T] int32) (mml_pcgrad_weights)."""
    _need_gpu(gram, order)
    T = gram.shape[0]
    if gram.dtype != torch.float64 or order.dtype != torch.int32 or order.numel() != T * T or gram.numel() != T * T \
            or not gram.is_contiguous() or not order.is_contiguous():
        raise L.MMLError("pcgrad_weights: gram [T, T] float64 and order [T, T] int32, contiguous")
    if w is None:
        w = torch.empty(2 * T, dtype=torch.float32, device=gram.device)
    if fired is None:
        fired = torch.empty((T, T), dtype=torch.int32, device=gram.device)
    _issue(bind.pcgrad_weights(gram, order, T, w, fired))
    return w, fired


def pcgrad_combine(segs, T, w):
    """out = sum_k w'[k] bank_k for every segment: the mean weights where every bank is there, the sum weights otherwise
    (mml_pcgrad_combine)."""
    _need_gpu(w)
    arr = make_pcgrad_segs(segs, T, need_out=True)
    _issue(bind.pcgrad_combine(arr, len(segs), T, w))


def act_bwd(y, dy, dst, act):
    _issue(bind.act_bwd(y, dy, dst, act))


# ---------------------------------------------------------------------------------------------- K8
def make_hyper(kind, lr, step=1, step_dev=None, zero_grad=False, max_blocks=0, cold_loop=0):
    """cold_loop: mml_opt_hyper.cold_loop (1 = the byte-walking loop over a warm map, for A/B runs)."""
    h = L.OptHyper()
    h.cold_loop = int(cold_loop)
    h.kind = L.OPT_KINDS[kind] if isinstance(kind, str) else int(kind)
    h.step = int(step)
    h.step_dev = L.ptr(step_dev)
    h.lr = float(lr)
    h.beta1, h.beta2 = 0.9, 0.999
    h.eps = {L.OPT_ADAM: 1e-8, L.OPT_ADAGRAD: 1e-10, L.OPT_RMSPROP: 1e-8}.get(h.kind, 0.0)
    h.alpha = 0.99
    h.zero_grad = int(zero_grad)
    h.max_blocks = int(max_blocks)
    return h


def make_opt_tensors(entries):
    """entries: (param, grad, state1 or None, state2 or None[, (l1, l2)[, skip bitmap[, gradient marks[, totals]]]]) with
    equal element counts, contiguous.  A skip bitmap (int32 words, one bit per table row) turns the entry into the untouched-rows half of the
    split dense table update (include/mmlrec.h: mml_opt_tensor.skip_rows).  totals = (acc64 tensor, magnitude slot,
    scatter_det_shift(B)): the deferred row totals of the deterministic scatter (mml_opt_tensor.acc64).  A ninth
    element, the warm map (uint8, one byte per table row, kept with the moments: mml_opt_tensor.warm_rows), lets a marked
    launch pass over the rows whose moments are still zero; it goes with gradient marks only."""
    arr = (L.OptTensor * len(entries))()
    for d, ent in zip(arr, entries):
        p, g, s1, s2 = ent[:4]
        d.param, d.grad, d.state1, d.state2, d.n = p.data_ptr(), g.data_ptr(), L.ptr(s1), L.ptr(s2), p.numel()
        d.l1, d.l2 = ent[4] if len(ent) > 4 and ent[4] else (0.0, 0.0)
        if len(ent) > 5 and ent[5] is not None:
            d.skip_rows, d.row_elems, d.zero_grads = ent[5].data_ptr(), p.shape[1], 1
        if len(ent) > 6 and ent[6] is not None:  # byte marks of the rows whose gradient is non-zero (uint8 view)
            d.grad_marks, d.row_elems = ent[6].data_ptr(), p.shape[1]
        if len(ent) > 7 and ent[7] is not None:
            d.acc64, d.acc_amax, d.acc_shift = ent[7][0].data_ptr(), ent[7][1].data_ptr(), int(ent[7][2])
        if len(ent) > 8 and ent[8] is not None:
            d.warm_rows = ent[8].data_ptr()
    return arr


def opt_step_dense(entries, hyper):
    arr = make_opt_tensors(entries)
    L.check(L.load().mml_opt_step_dense(arr, len(entries), C.byref(hyper), _stream()), "mml_opt_step_dense")


def opt_step_rows(tables, grad_tables, state1, state2, seen, rowbase, touched, touched_count, hyper, last=None):
    _issue(bind.opt_step_rows(tables, grad_tables, state1, state2,
                              bind.rows_args(None, seen, rowbase, touched, touched_count), hyper, last))


def index_unique(vocab, cols, E, X, seen, rowbase, touched, touched_count, status=None, marks=None):
    _issue(bind.index_unique(vocab, cols, E, X, bind.rows_args(None, seen, rowbase, touched, touched_count, marks), status))


def opt_catchup_rows(tables, state1, state2, last, rowbase, touched, touched_count, hyper):
    _issue(bind.opt_catchup_rows(tables, state1, state2, last, bind.rows_args(None, None, rowbase, touched, touched_count),
                                 hyper))


def opt_catchup_dense(table, state1, state2, last, hyper):
    L.check(L.load().mml_opt_catchup_dense(table.data_ptr(), L.ptr(state1), L.ptr(state2), last.data_ptr(),
                                           table.shape[0], table.shape[1], C.byref(hyper), _stream()),
            "mml_opt_catchup_dense")


def counter_update(counter, delta=1, reset=False):
    _issue(bind.counter_update(counter, delta, reset))


def step_counter(device):
    """(step_dev, consts): a device step counter and, in the same allocation (so neither outlives the other), the 16
    aligned bytes mml_opt_step_begin keeps the step's constants in (mml_opt_step_consts)."""
    buf = torch.zeros(8, dtype=torch.int32, device=device)
    return buf[:1], buf[4:8]


def opt_step_begin(step_dev, hyper, consts, delta=1):
    """*step_dev += delta and the new step's constants into `consts` in one launch; from here on the optimizer launches
    under step_dev and hyper's kind / lr / betas read them there (include/mmlrec.h: mml_opt_step_begin)."""
    L.check(L.load().mml_opt_step_begin(step_dev.data_ptr(), int(delta), C.byref(hyper), consts.data_ptr(), _stream()),
            "mml_opt_step_begin")


def opt_step_unbind(step_dev):
    L.check(L.load().mml_opt_step_unbind(step_dev.data_ptr()), "mml_opt_step_unbind")


def auc_segments(pred, y, seg):
    """AUC of every (segment of `seg` rows, column) pair of device matrices pred / y [n, C] -> float64 [ceil(n/seg), C]
    (NaN where a segment holds one class).  Device counterpart of the per-step sklearn roc_auc_score of the reference
    loop (model/basemodel.py:316-331)."""
    lib = L.load()
    n, c = pred.shape
    out = torch.empty(((n + seg - 1) // seg, c), dtype=torch.float64, device=pred.device)
    L.check(lib.mml_auc_segments(pred.data_ptr(), pred.stride(0), y.data_ptr(), y.stride(0), n, c, int(seg),
                                 out.data_ptr(), _stream()), "mml_auc_segments")
    return out


AUC_STATUS_NONFINITE = 16  # bit 4 of mml_auc_sorted's status word: a NaN / infinite score at a participating row


def auc_key_image(score):
    """The 32-bit order-preserving image of an fp32 score that mml_auc_sorted sorts by (csrc/auc_sort.hip, auc_image):
    -0.0 becomes +0.0, negative floats have all bits flipped, the others get the sign bit set.  a < b as floats
    <=> image(a) < image(b) as unsigned integers, and a == b <=> equal images.  Pure Python, for tests and docs."""
    import struct
    u, = struct.unpack("<I", struct.pack("<f", float(score)))
    if u == 0x80000000:
        u = 0
    return (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)


_auc_workspaces = {}


def _auc_workspace(device, n, cols, seg):
    """The workspace of one (device, stream, n, cols, seg): cached, a few shapes recur (evaluate's set, fit's epoch).  One
    per stream, because two calls that share a workspace must be ordered.  While a graph is being captured the buffer
    is allocated for that call instead (from the capture's memory pool, so it lives as long as the graph that holds its
    address): an entry of the cache may be evicted, a captured address may not."""
    nbytes = L.load().mml_auc_sorted_workspace_bytes(int(n), int(cols), int(seg))
    if nbytes < 0:
        raise L.MMLError(f"mml_auc_sorted: n * cols = {n} * {cols} keys, the call takes fewer than 2^31")
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=device)
    key = (device.type, device.index, _stream(), int(n), int(cols), int(seg))
    ws = _auc_workspaces.get(key)
    if ws is None:
        if len(_auc_workspaces) >= 8:  # (16 bytes per key each: the oldest shape goes)
            _auc_workspaces.pop(next(iter(_auc_workspaces)))
        ws = torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=device)
        _auc_workspaces[key] = ws
    return ws


def auc_sorted(pred, y, seg=0, mask=None, return_counts=False, status=None):
    """AUC of every (segment of `seg` rows, column) pair of device matrices pred / y [n, C] -> float64 [segments, C], for
    segments of ANY length (seg = 0: the whole set is one segment) -- mml_auc_sorted, a multi-workgroup radix sort.
    mask [n, 1] or [n, C] float32: a row takes part in a column iff its mask entry is non-zero (masked_select before
    scoring).  NaN where a problem holds one class, no row, or a non-finite score at a participating row; the latter
    also sets AUC_STATUS_NONFINITE in `status` (a device int32 tensor of one element the caller cleared; optional).
    return_counts: also the int64 [segments, C, 3] tensor of (2U, P, N), the integers the AUC is formed from."""
    _need_gpu(pred, y, mask, status)
    lib = L.load()
    pred, y = _f32_2d(pred, "pred"), _f32_2d(y, "y")
    n, c = pred.shape
    if tuple(y.shape) != (n, c):
        raise L.MMLError(f"auc_sorted: pred {tuple(pred.shape)} and y {tuple(y.shape)} differ")
    seg = int(seg)
    if seg <= 0 or seg >= n:
        seg = 0
    nseg = 1 if seg == 0 else (n + seg - 1) // seg
    mask_cols = 0
    if mask is not None:
        mask = _f32_2d(mask, "mask")
        mask_cols = mask.shape[1]
        if mask.shape[0] != n:
            raise L.MMLError(f"auc_sorted: mask has {mask.shape[0]} rows, pred {n}")
    out = torch.empty((nseg, c), dtype=torch.float64, device=pred.device)
    counts = torch.empty((nseg, c, 3), dtype=torch.int64, device=pred.device) if return_counts else None
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=pred.device)
    ws = _auc_workspace(pred.device, n, c, seg)
    L.check(lib.mml_auc_sorted(pred.data_ptr(), _ld(pred), y.data_ptr(), _ld(y), L.ptr(mask),
                               _ld(mask) if mask is not None else 0, mask_cols, n, c, seg, ws.data_ptr(), ws.numel(),
                               out.data_ptr(), L.ptr(counts), status.data_ptr(), _stream()), "mml_auc_sorted")
    return (out, counts) if return_counts else out


# ---------------------------------------------------------------------------------------------- K3' (bf16 storage)
def _is16(t):
    return t.dtype == torch.bfloat16


def _need16(t, name):
    if t.dtype != torch.bfloat16 or t.dim() != 2 or t.stride(1) != 1:
        raise L.MMLError(f"{name}: expected a bf16 2-D tensor with unit inner stride, got {t.dtype} {tuple(t.shape)}")
    return t


def make_cast16_descs(items):
    """items: (src fp32 [r, c], dst bf16 [r, c] or, transposed, [c, r], transpose flag)."""
    arr = (L.Cast16Desc * len(items))()
    for d, (src, dst, tr) in zip(arr, items):
        _f32_2d(src, "cast16 source")
        _need16(dst, "cast16 destination")
        want = (src.shape[1], src.shape[0]) if tr else tuple(src.shape)
        if tuple(dst.shape) != want:
            raise L.MMLError(f"cast16: destination shape {tuple(dst.shape)}, expected {want}")
        d.src, d.dst, d.rows, d.cols = src.data_ptr(), dst.data_ptr(), src.shape[0], src.shape[1]
        d.lds, d.ldd, d.transpose = _ld(src), _ld(dst), int(bool(tr))
    return arr


def cast16(src, transpose=False, out=None):
    _need_gpu(src)
    if out is None:
        shape = (src.shape[1], src.shape[0]) if transpose else tuple(src.shape)
        out = torch.empty(shape, dtype=torch.bfloat16, device=src.device)
    arr = make_cast16_descs([(src, out, transpose)])
    L.check(L.load().mml_cast16_batch(arr, 1, _stream()), "mml_cast16_batch")
    return out


def gather16_fwd(tables, X, cols, dense_col0=0, nd=0, out=None, status=None):
    """gather_fwd writing dnn_input as bf16 (mml_gather16_fwd)."""
    _need_gpu(X, *tables)
    X = _f32_2d(X, "X")
    if out is None:
        out = torch.empty((X.shape[0], len(tables) * tables[0].shape[1] + nd), dtype=torch.bfloat16, device=X.device)
    _issue(bind.gather16_fwd(tables, X, cols, dense_col0, nd, out, status))
    return out


def make_g16_tn_descs(problems):
    """problems: dicts with srcs [(A bf16 [M, K_s], B bf16 [N, K_s]), ...], C ([M, N] bf16 or fp32), optional bias [N]
    fp32, act, accumulate, mask_out / mask_in (int32 [M, ceil(N / 32)])."""
    arr = (L.G16TnDesc * len(problems))()
    for d, q in zip(arr, problems):
        Cm = q["C"]
        d.M, d.N = Cm.shape
        d.n_src = len(q["srcs"])
        if not 1 <= d.n_src <= L.MAX_SRC:
            raise L.MMLError("g16_tn: 1 .. MAX_SRC sources")
        for s, (A, Bm) in enumerate(q["srcs"]):
            _need16(A, "g16_tn A")
            _need16(Bm, "g16_tn B")
            if A.shape[0] != d.M or Bm.shape[0] != d.N or A.shape[1] != Bm.shape[1]:
                raise L.MMLError(f"g16_tn: source {s} shapes {tuple(A.shape)} x {tuple(Bm.shape)} for C {tuple(Cm.shape)}")
            d.A[s], d.B[s], d.lda[s], d.ldb[s], d.K[s] = A.data_ptr(), Bm.data_ptr(), _ld(A), _ld(Bm), A.shape[1]
        d.act = int(q.get("act", L.ACT_NONE))
        d.bias = L.ptr(q.get("bias"))
        d.C, d.ldc, d.c_bf16 = Cm.data_ptr(), _ld(Cm), int(_is16(Cm))
        if not d.c_bf16 and Cm.dtype != torch.float32:
            raise L.MMLError("g16_tn: C must be bf16 or fp32")
        d.accumulate = int(q.get("accumulate", 0))
        mo, mi = q.get("mask_out"), q.get("mask_in")
        d.mask_out, d.mask_in = L.ptr(mo), L.ptr(mi)
        m = mo if mo is not None else mi
        d.ldmask = _ld(m) if m is not None else 0
    return arr


def g16_tn(problems):
    arr = make_g16_tn_descs(problems)
    L.check(L.load().mml_g16_tn(arr, len(problems), _stream()), "mml_g16_tn")


def make_g16_wgrad_descs(problems):
    """problems: dicts with dC bf16 [M, N], A bf16 [M, K], dW fp32 [N, K], optional dbias fp32 [N], accumulate."""
    arr = (L.G16WgradDesc * len(problems))()
    for d, q in zip(arr, problems):
        dC, A, dW = _need16(q["dC"], "g16_wgrad dC"), _need16(q["A"], "g16_wgrad A"), _f32_2d(q["dW"], "g16_wgrad dW")
        d.M, d.N, d.K = dC.shape[0], dC.shape[1], A.shape[1]
        if A.shape[0] != d.M or tuple(dW.shape) != (d.N, d.K):
            raise L.MMLError("g16_wgrad: shape mismatch")
        d.dC, d.A, d.dW, d.dbias = dC.data_ptr(), A.data_ptr(), dW.data_ptr(), L.ptr(q.get("dbias"))
        d.lddc, d.lda, d.lddw = _ld(dC), _ld(A), _ld(dW)
        d.accumulate = int(q.get("accumulate", 0))
    return arr


def g16_wgrad(problems, phases=False):
    lib = L.load()
    arr = make_g16_wgrad_descs(problems)
    n = int(lib.mml_g16_wgrad_workspace_bytes(arr, len(problems)))
    if n < 0:
        L.check(-1, "mml_g16_wgrad_workspace_bytes")
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device=problems[0]["dW"].device)
    for ph in ((1, 2) if phases else (0,)):
        L.check(lib.mml_g16_wgrad(arr, len(problems), ws.data_ptr(), ws.numel(), ph, _stream()), "mml_g16_wgrad")
