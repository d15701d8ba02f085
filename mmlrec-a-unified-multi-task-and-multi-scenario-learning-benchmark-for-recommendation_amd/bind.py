"""The argument order of the C entry points that take four or more positional arguments (include/mmlrec.h), written
ONCE per entry point: the row family (gather, scatter, index-unique, rows bookkeeping, row optimizer) and the model layer
(BatchNorm, dropout, APG, SNR, ESMM / ESCM, the element-wise and copy kernels, PCGrad, counters).  A builder takes
tensors (or ctypes arrays and structures already built) plus sizes and flags and returns Bound(name, args): the C symbol
and its positional arguments without the trailing stream.  Two consumers: the eager wrappers (ops._issue) and the
recorded plans (engine.Plan.bound).  Marshalling only -- no checks, no allocation, no device work -- so the builders also
run on host tensors (the CPU restatement of the C ABI, tests/test_bind_cpu.py, tests/test_bind_model_cpu.py).  Entry points
whose whole list is (descriptor array, count) or (byref(group), workspace, bytes) are written where they are used.
A Bound holds ADDRESSES: whoever records one keeps the tensors alive (Plan.bound keeps only the ctypes objects).

Conventions: `tables` = the [V, E] tensors of the fields (their order is the field order), `X` = the [B, ldX] fp32-encoded
index matrix, `rows` = the bookkeeping tuple of rows_args, `d` = an mml_pool_desc (ops.make_pool_desc), `B` = the rows of
X to read when not all of them.  Model layer: rows, columns and pitches come from the 2-D views given (`ld`); `ws` = a
uint8 workspace tensor, which supplies its address and its byte count; `acc` / `accumulate` = add to the output."""
import collections
import ctypes as C

from . import _lib as L

Bound = collections.namedtuple("Bound", "name args")


def ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _mat(t):
    """(address, row pitch) of a 2-D view: how the header passes every matrix; (null, 0) for None."""
    return (None, 0) if t is None else (t.data_ptr(), ld(t))


def _ptrs(*tensors):
    return tuple(L.ptr(t) for t in tensors)


def ptr_array(tensors):
    """void* array of the tensors' addresses (None entries stay null); None and a built array pass through."""
    if tensors is None or isinstance(tensors, C.Array):
        return tensors
    arr = (L.fp * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr() if t is not None else None
    return arr


def _ints(ctype, values):
    if values is None or isinstance(values, C.Array):
        return values
    values = list(values)
    return (ctype * len(values))(*values)


def _nrows(X, B):
    return X.shape[0] if B is None else B


def rows_args(rows=None, seen=None, rowbase=None, touched=None, count=None, marks=None):
    """The touched-row bookkeeping of a scatter / index-unique call: (seen[], rowbase, touched, count, cap, row_marks),
    from a TableRows-like object (`rows`, which then supplies all five) or from loose tensors; whatever is not given is
    null: rows_args() = no bookkeeping, rows_args(None, marks=m) = the marks alone."""
    if rows is not None:
        seen, rowbase, touched, count, marks = rows.seen, rows.rowbase, rows.touched, rows.count, rows.marks
    return (ptr_array(seen), _ints(L.i64, rowbase), L.ptr(touched), L.ptr(count),
            0 if touched is None else touched.numel(), L.ptr(marks))


def _fields(tables, cols):
    """(tables[], vocab[], cols[], F, E): how every per-field entry point opens."""
    return (ptr_array(tables), _ints(L.i64, [t.shape[0] for t in tables]), _ints(L.i32, cols), len(tables),
            tables[0].shape[1])


# ---------------------------------------------------------------------------------------------- gather
def _gather(name, tables, X, cols, dense_col0, nd, out, tail, B):
    return Bound(name, _fields(tables, cols) + (X.data_ptr(), ld(X), dense_col0, nd, _nrows(X, B), out.data_ptr(),
                                                ld(out)) + tail)


def gather_fwd(tables, X, cols, dense_col0, nd, out, status=None, B=None):
    return _gather("mml_gather_fwd", tables, X, cols, dense_col0, nd, out, (L.ptr(status),), B)


def gather16_fwd(tables, X, cols, dense_col0, nd, out, status=None, B=None):
    return _gather("mml_gather16_fwd", tables, X, cols, dense_col0, nd, out, (L.ptr(status),), B)


def gather_fwd_wgmax(tables, X, cols, dense_col0, nd, out, wg, n_wg, status=None, B=None):
    return _gather("mml_gather_fwd_wgmax", tables, X, cols, dense_col0, nd, out, (wg.data_ptr(), n_wg, L.ptr(status)), B)


def gather_fwd_mark(tables, X, cols, dense_col0, nd, out, marks, status=None, B=None):
    return _gather("mml_gather_fwd_mark", tables, X, cols, dense_col0, nd, out, (marks.data_ptr(), L.ptr(status)), B)


def gather_fwd_idx32(tables, idx, dense, out, status=None):
    """idx: native int32 [B, F]; dense: the [B, nd] columns copied behind the blocks, or None."""
    F = len(tables)
    return Bound("mml_gather_fwd_idx32",
                 (ptr_array(tables), _ints(L.i64, [t.shape[0] for t in tables]), F, tables[0].shape[1], idx.data_ptr(),
                  idx.stride(0), L.ptr(dense), 0 if dense is None else dense.stride(0),
                  0 if dense is None else dense.shape[1], idx.shape[0], out.data_ptr(), ld(out), L.ptr(status)))


def gather_pool_fwd(d, X, dense_col0, nd, out, argmax=None, wg=None, n_wg=0, status=None, B=None):
    return Bound("mml_gather_pool_fwd",
                 (C.byref(d), X.data_ptr(), ld(X), dense_col0, nd, _nrows(X, B), out.data_ptr(), ld(out)) + _mat(argmax) +
                 (L.ptr(wg), n_wg, L.ptr(status)))


# ---------------------------------------------------------------------------------------------- scatter
def scatter_bwd(grad_tables, X, cols, d_out, rows, status=None, B=None):
    return Bound("mml_scatter_bwd", _fields(grad_tables, cols) + (X.data_ptr(), ld(X), _nrows(X, B), d_out.data_ptr(),
                                                                 ld(d_out)) + rows + (L.ptr(status),))


def scatter_bwd_det(grad_tables, X, cols, d_out, acc64, amax_slot, marks, flags, status=None, B=None):
    return Bound("mml_scatter_bwd_det",
                 _fields(grad_tables, cols) + (X.data_ptr(), ld(X), _nrows(X, B), d_out.data_ptr(), ld(d_out),
                                               ptr_array(acc64), amax_slot.data_ptr(), L.ptr(marks), int(flags),
                                               L.ptr(status)))


def scatter_bwd_idx32(grad_tables, idx, d_out, rows, status=None):
    F = len(grad_tables)
    return Bound("mml_scatter_bwd_idx32",
                 (ptr_array(grad_tables), _ints(L.i64, [t.shape[0] for t in grad_tables]), F, grad_tables[0].shape[1],
                  idx.data_ptr(), idx.stride(0), idx.shape[0], d_out.data_ptr(), ld(d_out)) + rows + (L.ptr(status),))


def scatter_pool_bwd(d, X, d_out, argmax, rows, status=None, B=None):
    return Bound("mml_scatter_pool_bwd",
                 (C.byref(d), X.data_ptr(), ld(X), _nrows(X, B), d_out.data_ptr(), ld(d_out)) + _mat(argmax) + rows +
                 (L.ptr(status),))


def scatter_pool_bwd_det(d, X, d_out, argmax, acc64, amax_slot, marks, flags, status=None, B=None):
    return Bound("mml_scatter_pool_bwd_det",
                 (C.byref(d), X.data_ptr(), ld(X), _nrows(X, B), d_out.data_ptr(), ld(d_out)) + _mat(argmax) +
                 (ptr_array(acc64), amax_slot.data_ptr(), L.ptr(marks), int(flags), L.ptr(status)))


# ---------------------------------------------------------------------------------------------- rows bookkeeping
def index_unique(vocab, cols, E, X, rows, status=None, B=None):
    return Bound("mml_index_unique", (_ints(L.i64, vocab), _ints(L.i32, cols), len(vocab), E, X.data_ptr(), ld(X),
                                      _nrows(X, B)) + rows + (L.ptr(status),))


def index_unique_pool(d, X, rows, status=None, B=None):
    return Bound("mml_index_unique_pool", (C.byref(d), X.data_ptr(), ld(X), _nrows(X, B)) + rows + (L.ptr(status),))


def rows_compact(vocab, rows):
    """The marks a marking kernel left -> `seen` bitmaps + touched list (clears the marks)."""
    return Bound("mml_rows_compact", (rows[0], _ints(L.i64, vocab), rows[1], len(vocab)) + rows[2:])


# ---------------------------------------------------------------------------------------------- row optimizer
def opt_step_rows(tables, grad_tables, state1, state2, rows, hyper, last=None):
    """state1 / state2 / last: one tensor per table, or None for what the optimizer kind does not keep."""
    return Bound("mml_opt_step_rows",
                 (ptr_array(tables), ptr_array(grad_tables), ptr_array(state1), ptr_array(state2), rows[0], rows[1],
                  len(tables), tables[0].shape[1], rows[2], rows[3], rows[4], ptr_array(last), C.byref(hyper)))


def opt_catchup_rows(tables, state1, state2, last, rows, hyper):
    return Bound("mml_opt_catchup_rows",
                 (ptr_array(tables), ptr_array(state1), ptr_array(state2), ptr_array(last), rows[1], len(tables),
                  tables[0].shape[1], rows[2], rows[3], rows[4], C.byref(hyper)))


# ---------------------------------------------------------------------------------------------- BatchNorm
def bn_fwd(x, gamma, beta, running_mean, running_var, batches_tracked, mean, rstd, y, act, training, eps, momentum, ws):
    return Bound("mml_bn_fwd", _mat(x) + _ptrs(gamma, beta, running_mean, running_var, batches_tracked, mean, rstd) + _mat(y) +
                 tuple(x.shape) + (int(act), int(training), float(eps), float(momentum), ws.data_ptr(), ws.numel()))


def bn_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, acc, ws):
    return Bound("mml_bn_bwd", _mat(dy) + _mat(x) + _ptrs(gamma, mean, rstd) + _mat(dx) + _ptrs(dgamma, dbeta) +
                 (int(acc),) + tuple(x.shape) + (ws.data_ptr(), ws.numel()))


def domain_bn_update(x, mask, pop_mean, pop_var, decay):
    """mask: [B, D] one-hot rows; pop_mean / pop_var: [D, n]."""
    return Bound("mml_domain_bn_update", _mat(x) + _mat(mask) + tuple(x.shape) + (mask.shape[1],) +
                 _ptrs(pop_mean, pop_var) + (float(decay),))


def domain_bn_eval(x, mask, pop_mean, pop_var, y, eps):
    return Bound("mml_domain_bn_eval", _mat(x) + _mat(mask) + _ptrs(pop_mean, pop_var) + _mat(y) + tuple(x.shape) +
                 (mask.shape[1], float(eps)))


# ---------------------------------------------------------------------------------------------- dropout
def dropout(x, out, p, seed, site, step_dev, step, accumulate, row0, rows=None):
    """seed / site: any Python int, cut to the 64 / 32 bits the mask stream takes -- here, once; step_dev: the device
    step counter (then `step` is not read) or None."""
    return Bound("mml_dropout", _mat(x) + _mat(out) + (_nrows(x, rows), x.shape[1], int(row0), float(p),
                                                       int(seed) & ((1 << 64) - 1), int(site) & 0xffffffff,
                                                       L.ptr(step_dev), int(step), int(accumulate)))


# ---------------------------------------------------------------------------------------------- APG
def apg_features_fwd(o1, s, z, k, E):
    return Bound("mml_apg_features_fwd", _mat(o1) + _mat(s) + _mat(z) + (o1.shape[0], k, E, z.shape[1]))


def apg_features_bwd(dz, s, do1, k, E, acc):
    return Bound("mml_apg_features_bwd", _mat(dz) + _mat(s) + _mat(do1) + (dz.shape[0], k, E, int(acc)))


def apg_weights(Wkk, bkk, Wb, Wcat, k, E, direction, acc=(0, 0, 0)):
    """direction 0: pack Wcat from the three; 1: unpack (the four are then the gradients), acc = one flag per target.
    Wcat's pitch is k."""
    return Bound("mml_apg_weights", _ptrs(Wkk, bkk, Wb, Wcat) + (k, k, E, int(direction)) + tuple(acc))


# ---------------------------------------------------------------------------------------------- SNR
def snr_gate_weights_fwd(u, alpha, M, W, n_blocks, block, zw, beta, gamma, eps):
    return Bound("mml_snr_gate_weights_fwd", _ptrs(u, alpha, M, W) + (n_blocks, block, zw, float(beta), float(gamma), float(eps)))


def snr_gate_weights_bwd(dW, M, u, alpha, du, dalpha, acc_u, acc_alpha, n_blocks, block, zw, beta, gamma, eps, scratch):
    """du: None for a frozen u; scratch: n_blocks floats."""
    return Bound("mml_snr_gate_weights_bwd", _ptrs(dW, M, u, alpha, du, dalpha) + (int(acc_u), int(acc_alpha), n_blocks, block,
                                                                                   zw, float(beta), float(gamma), float(eps),
                                                                                   scratch.data_ptr()))


# ---------------------------------------------------------------------------------------------- ESMM / ESCM
def _combine(name, raw, y, dout, prob, draw, loss, B, tail=()):
    return Bound(name, _mat(raw) + _mat(y) + _mat(dout) + _mat(prob) + _mat(draw) + (L.ptr(loss), B) + tail)


def esmm_combine(raw, y, dout, prob, draw, loss, B):
    """y / dout / draw / loss: None for what the pass does not read or write."""
    return _combine("mml_esmm_combine", raw, y, dout, prob, draw, loss, B)


def escm_combine(raw, y, dout, prob, draw, loss, B, cf_w, global_w):
    return _combine("mml_escm_combine", raw, y, dout, prob, draw, loss, B, (float(cf_w), float(global_w)))


# ---------------------------------------------------------------------------------------------- element-wise
def ew_mul(a, b, out):
    return Bound("mml_ew_mul", _ptrs(a, b, out) + (out.numel(),))


def ew_mul_bwd(dout, a, b, da, db, acc_a, acc_b):
    return Bound("mml_ew_mul_bwd", _ptrs(dout, a, b, da, db) + (int(acc_a), int(acc_b), dout.numel()))


def ew_mul_bwd_act(dout, a, b, da, db, acc_a, acc_b, act_a, act_b):
    return Bound("mml_ew_mul_bwd_act", ew_mul_bwd(dout, a, b, da, db, acc_a, acc_b).args + (int(act_a), int(act_b)))


def ew_add_n(inputs, out, n=None):
    """n: the flat extent when it is not out's own (rows of a padded pitch); likewise act_bwd."""
    arr = ptr_array(inputs)
    return Bound("mml_ew_add_n", (arr, len(arr), out.data_ptr(), out.numel() if n is None else n))


def act_bwd(y, dy, dst, act, n=None):
    return Bound("mml_act_bwd", _ptrs(y, dy, dst) + (y.numel() if n is None else n, int(act)))


def copy2d(src, dst, accumulate):
    """dst (+)= src over src's [rows, cols].  (passes.merge_copies reads this layout positionally.)"""
    return Bound("mml_copy2d", _mat(src) + _mat(dst) + tuple(src.shape) + (int(accumulate),))


def copy_flat(src, dst, accumulate, n=None):
    """The same entry point over n contiguous elements of tensors of any rank: one row of n columns."""
    n = src.numel() if n is None else n
    return Bound("mml_copy2d", (src.data_ptr(), n, dst.data_ptr(), n, 1, n, int(accumulate)))


# ---------------------------------------------------------------------------------------------- PCGrad
def pcgrad_gram(arr, n, T, gram, ws):
    """arr: an mml_pcgrad_seg array (ops.make_pcgrad_segs) of n segments."""
    return Bound("mml_pcgrad_gram", (arr, n, T, gram.data_ptr(), ws.data_ptr(), ws.numel()))


def pcgrad_weights(gram, order, T, w, fired):
    return Bound("mml_pcgrad_weights", _ptrs(gram, order) + (T,) + _ptrs(w, fired))


def pcgrad_combine(arr, n, T, w):
    return Bound("mml_pcgrad_combine", (arr, n, T, w.data_ptr()))


def pcgrad_stash(arr, n, tables):
    """tables: the segments are table gradients -- the rows copied are zeroed behind the copy (the header's `clear`)."""
    return Bound("mml_pcgrad_stash", (arr, n, int(tables)))


# ---------------------------------------------------------------------------------------------- counters
def counter_update(counter, delta, reset):
    return Bound("mml_counter_update", (counter.data_ptr(), int(delta), int(reset)))


def amax_reset(pool, n):
    """Zero the first n magnitude slots of the pool."""
    return Bound("mml_amax_reset", (pool.data_ptr(), int(n)))
