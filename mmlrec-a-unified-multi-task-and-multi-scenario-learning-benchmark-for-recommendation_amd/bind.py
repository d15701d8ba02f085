"""The argument order of the row-family entry points (include/mmlrec.h: gather, scatter, index-unique, rows bookkeeping,
row optimizer), written ONCE per entry point.  A builder takes tensors (or ctypes arrays already built) plus sizes and
returns Bound(name, args): the C symbol and its positional arguments without the trailing stream.  Two consumers:
the eager wrappers (ops._issue) and the recorded plans (engine.Plan.bound).  Marshalling only -- no checks, no allocation,
no device work -- so the builders also run on host tensors (the CPU restatement of the C ABI, tests/test_bind_cpu.py).

Conventions: `tables` = the [V, E] tensors of the fields (their order is the field order), `X` = the [B, ldX] fp32-encoded
index matrix, `rows` = the bookkeeping tuple of rows_args, `d` = an mml_pool_desc (ops.make_pool_desc), `B` = the rows of
X to read when not all of them."""
import collections
import ctypes as C

from . import _lib as L

Bound = collections.namedtuple("Bound", "name args")


def ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


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


def _ld_or_0(t):
    return 0 if t is None else ld(t)


def gather_pool_fwd(d, X, dense_col0, nd, out, argmax=None, wg=None, n_wg=0, status=None, B=None):
    return Bound("mml_gather_pool_fwd",
                 (C.byref(d), X.data_ptr(), ld(X), dense_col0, nd, _nrows(X, B), out.data_ptr(), ld(out), L.ptr(argmax),
                  _ld_or_0(argmax), L.ptr(wg), n_wg, L.ptr(status)))


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
                 (C.byref(d), X.data_ptr(), ld(X), _nrows(X, B), d_out.data_ptr(), ld(d_out), L.ptr(argmax),
                  _ld_or_0(argmax)) + rows + (L.ptr(status),))


def scatter_pool_bwd_det(d, X, d_out, argmax, acc64, amax_slot, marks, flags, status=None, B=None):
    return Bound("mml_scatter_pool_bwd_det",
                 (C.byref(d), X.data_ptr(), ld(X), _nrows(X, B), d_out.data_ptr(), ld(d_out), L.ptr(argmax),
                  _ld_or_0(argmax), ptr_array(acc64), amax_slot.data_ptr(), L.ptr(marks), int(flags), L.ptr(status)))


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
