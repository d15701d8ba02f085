"""Kernel-level tests of four entry points every training step depends on -- mml_sumprod_batch (csrc/ew.hip),
mml_gather_fwd_mark and mml_rows_compact (csrc/gather_scatter.hip), mml_shard_rows (csrc/shard.hip) -- and of the small
elementwise neighbours of sumprod (mml_ew_mul, mml_ew_mul_bwd, mml_ew_mul_bwd_act, mml_ew_add_n, mml_act_bwd,
mml_copy2d) against the host references of tests/row_kernel_refs.py (proved by tests/test_row_kernel_refs_cpu.py).
Every call goes through _lib.load() with raw pointers.  Every output buffer, the words in front of an offset pointer and
a guard region behind it are pre-filled with the quiet-NaN sentinel 0x7FC5A5A5 (byte maps: 0xA5 guard bytes, int32 lists:
the word 0xA5A5A5A5); only the elements the contract names may change, and every input must keep its bits.

Worst observed err / (tol * sum|terms|) per case family on an MI355X (first device run; printed again at the end of
every run with -s).  The bit-equality checks (every index, list, bitmap, mark and shard comparison, mml_ew_mul,
mml_ew_add_n, mml_copy2d, mml_ew_mul_bwd without accumulation, sumprod with at most one rounding) have no ratio.
  mml_sumprod_batch lengths      0.446   tol (n_terms + 4) 2^-24
  mml_sumprod_batch paths        0.383   (the two paths against each other as well as against the reference)
  mml_sumprod_batch terms        0.343
  mml_sumprod_batch activation   0.446
  mml_sumprod_batch blocks       0.480
  mml_sumprod_batch amax         0.397
  mml_ew_mul_bwd (accumulating)  0.890   of 2 x 2^-24: the product and the add are rounded separately
  mml_ew_mul_bwd_act             0.786   of 4 x 2^-24
  mml_act_bwd                    0.584   of 4 x 2^-24
No case failed on the device and no kernel was changed.  The one defect was found by reading: mml_sumprod_batch validated
and launched block by block of 16 items, so a malformed item 16 was reported after items 0..15 had been overwritten.  It
now validates the whole array before its first launch (host code of csrc/ew.hip only);
test_sumprod_rejections_write_nothing[*-16] fails on a library with the former host code and passes on this one.

Sensitivity on the device (once, while writing this file): libraries built with one in-bounds mutation each failed
exactly the tests that cover it and no other --
  rows_compact_kernel without `bits |= seen[wi]`     test_rows_compact (all but F1_V1, where the old bit is the new
                                                     mark), ..._short_list, ..._second_trip_of_the_workgroup_loop
  rows_compact_kernel clearing only m[0]             the same three (all but F1_V1 and V33, whose marks lie in the first
                                                     16 bytes of their words) and test_gather_mark_then_compact_is_index_unique
  sumprod_batch_kernel skipping the last term's y    every sumprod test with a 16-byte-path item whose last term has a y
  in the 16-byte path only                           (lengths, path_selection, terms[1028-*], activation[1028],
                                                     blocks_of_16[16, 17, 33], amax_slots); the scalar-path cases pass
  mml_sumprod_batch copying d[i] for d[i0 + i]       test_sumprod_blocks_of_16[17, 33], test_sumprod_terms (20 items),
                                                     test_sumprod_empty_block_and_empty_call
  shard_rows_kernel with r = l * world               test_shard_rows_to_shard / _to_table / _layout_of_row_sharding at
                                                     every world > 1
  the gather marking row + 1 (clamped to V - 1)      test_gather_fwd_mark (all but the six B = 1, V = 1 cases),
                                                     ..._out_of_range, ..._ignores_the_lds_variant, test_gather_mark_then_compact_...
"""
import numpy as np
import pytest
import torch

import row_kernel_refs as R
from row_kernel_refs import F32, F64, assert_close_terms, bits_equal

pytestmark = pytest.mark.gpu

SENT_BITS = np.uint32(0x7FC5A5A5)  # a quiet NaN with a payload no arithmetic produces
SENT_I32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
SENT_BYTE = 0xA5
GUARD = 8  # words (bytes x 8 for the byte maps) behind every buffer


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def env():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L
    from mmlrec_amd import ops
    R.RATIOS.clear()
    yield L.load(), L, ops
    print("\nworst err / (tol * sum|terms|):")
    for k in sorted(R.RATIOS):
        print(f"  {k:40s} {R.RATIOS[k]:.3f}")


@pytest.fixture()
def lib(env):
    return env[0]


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(lib, rc):
    assert rc == 0, (rc, lib.mml_last_error())


def refused(lib, rc, *needles):
    msg = (lib.mml_last_error() or b"").decode()
    assert rc != 0, "the call was accepted"
    for s in needles:
        assert s in msg, (s, msg)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


class Arr:
    """n float32 at element offset `off` of a device buffer of off + n + GUARD words; all other words are the sentinel."""

    def __init__(self, n, data=None, off=0):
        self.n, self.off = int(n), int(off)
        host = np.full(self.off + self.n + GUARD, SENT_BITS, np.uint32)
        if data is not None:
            host[self.off:self.off + self.n] = np.ascontiguousarray(data, dtype=F32).reshape(-1).view(np.uint32)
        self.before = host
        self.t = torch.from_numpy(host.view(F32).copy()).to(dev())
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.off

    def words(self):
        return self.t.cpu().numpy().view(np.uint32)

    def get(self, what):
        host = self.words()
        assert (host[:self.off] == SENT_BITS).all(), what + ": written in front of the array"
        assert (host[self.off + self.n:] == SENT_BITS).all(), what + ": written behind the array"
        return host[self.off:self.off + self.n].view(F32).copy()

    def unchanged(self):
        return np.array_equal(self.words(), self.before)


class Buf:
    """A [rows, cols] float32 matrix inside a [rows + 1, ld] device buffer whose every other element is the sentinel."""

    def __init__(self, rows, cols, ld=None, data=None):
        self.rows, self.cols, self.ld = rows, cols, cols if ld is None else ld
        host = np.full((rows + 1, self.ld), SENT_BITS, np.uint32)
        if data is not None:
            host[:rows, :cols] = np.ascontiguousarray(data, dtype=F32).reshape(rows, cols).view(np.uint32)
        self.before = host
        self.t = torch.from_numpy(host.view(F32).copy()).to(dev())

    @property
    def ptr(self):
        return self.t.data_ptr()

    def words(self):
        return self.t.cpu().numpy().view(np.uint32)

    def get(self, what):
        host = self.words()
        assert (host[:self.rows, self.cols:] == SENT_BITS).all(), what + ": a padding column was written"
        assert (host[self.rows] == SENT_BITS).all(), what + ": written behind the last row"
        return host[:self.rows, :self.cols].view(F32).copy()

    def unchanged(self):
        return np.array_equal(self.words(), self.before)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                 np.ascontiguousarray(b).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------
# 1. mml_sumprod_batch
# ---------------------------------------------------------------------------------------------------------------
class Item:
    """One item on the device.  off: element offsets of single operands ({"out": 1, ("x", 2): 1, ("y", 0): 1, "deriv": 1})
    -- an offset of one float takes the pointer off its 16-byte boundary."""

    def __init__(self, it, off=None, slot=None):
        off = off or {}
        n = it["n"]
        self.it, self.slot = it, slot
        self.xs = [Arr(n, x, off.get(("x", k), 0)) for k, x in enumerate(it["xs"])]
        self.ys = [None if y is None else Arr(n, y, off.get(("y", k), 0)) for k, y in enumerate(it["ys"])]
        self.out = Arr(n, it["prior"] if it["accumulate"] else None, off.get("out", 0))
        self.deriv = Arr(n, it["deriv_of"], off.get("deriv", 0)) if it["act"] else None

    def fill(self, d):
        d.out, d.n, d.n_terms, d.accumulate, d.act = self.out.ptr, self.it["n"], self.it["n_terms"], self.it["accumulate"], \
            self.it["act"]
        for k in range(R.SUMPROD_TERMS):
            d.x[k] = self.xs[k].ptr if k < len(self.xs) else None
            d.y[k] = self.ys[k].ptr if k < len(self.ys) and self.ys[k] is not None else None
        d.deriv_of = self.deriv.ptr if self.deriv is not None else None
        d.amax_out = self.slot.data_ptr() if self.slot is not None else None

    def inputs_unchanged(self):
        return all(a.unchanged() for a in self.xs + [y for y in self.ys if y is not None] +
                   ([self.deriv] if self.deriv is not None else []))

    def check(self, family, what):
        """the stored output against the float64 reference, element by element; bit equality where the arithmetic has at
        most one rounding"""
        it = self.it
        got = self.out.get(what)
        assert self.inputs_unchanged(), what + ": an input changed"
        ref, sa = R.ref64_sumprod_item(it)
        assert_close_terms(got, ref, sa, R.sumprod_tol(it["n_terms"]), f"mml_sumprod_batch {family}: {what}")
        exact = R.sumprod_exact32(it)
        if exact is not None:
            assert bits_equal(got, exact), what + ": not the float32 result"
        return got


def descs(L, items):
    arr = (L.SumProdDesc * max(len(items), 1))()
    for d, it in zip(arr, items):
        it.fill(d)
    return arr


def run_sumprod(env, items, family):
    lib, L, _ = env
    arr = descs(L, items)
    ok(lib, lib.mml_sumprod_batch(arr, len(items), stream()))
    return [it.check(family, f"item {i} (n={it.it['n']}, terms={it.it['n_terms']}, y={it.it['ypat']}, "
                             f"acc={it.it['accumulate']}, act={it.it['act']})") for i, it in enumerate(items)]


@pytest.mark.parametrize("accumulate", [0, 1])
def test_sumprod_lengths(env, accumulate):
    """n in {0, 1, 3, 4, 5, 1023, 1024, 4100} and, in the same 16-item block (grid capped at max(2048 / 16, 64) = 128
    workgroups), one scalar-path item of 33 001 elements and one 16-byte-path item of 140 004: both take a second
    grid-stride trip."""
    run_sumprod(env, [Item(it) for it in R.sumprod_length_items(accumulate)], "lengths")


def _truncated(it, n):
    cut = dict(it, n=n, xs=[x[:n] for x in it["xs"]], ys=[None if y is None else y[:n] for y in it["ys"]],
               prior=it["prior"][:n], deriv_of=None if it["deriv_of"] is None else it["deriv_of"][:n])
    return cut


PATH_VARIANTS = (("aligned", {}), ("out", {"out": 1}), ("x", {("x", 2): 1}), ("y", {("y", 0): 1}), ("deriv", {"deriv": 1}))


@pytest.mark.parametrize("mode", ["act", "accumulate", "plain"])
def test_sumprod_path_selection(env, mode):
    """Each condition of `vec` alone sends the item to the scalar path: n % 4 != 0 with everything aligned, `out`, one
    x[k], one y[k], deriv_of off its 16-byte boundary by one float.  Same data: both paths inside the tolerance of the
    reference and of each other."""
    base = R.sumprod_path_base(mode)
    variants = [(nm, off) for nm, off in PATH_VARIANTS if base["act"] or nm != "deriv"]
    items = [Item(base, off) for _, off in variants] + [Item(_truncated(base, 1023))]
    got = run_sumprod(env, items, "paths")
    _, sa = R.ref64_sumprod_item(base)
    for (nm, _), g in zip(variants[1:], got[1:-1]):
        assert_close_terms(g, got[0].astype(F64), sa, R.sumprod_tol(3), f"mml_sumprod_batch paths: scalar ({nm}) vs vec")
    assert_close_terms(got[-1], got[0][:1023].astype(F64), sa[:1023], R.sumprod_tol(3),
                       "mml_sumprod_batch paths: scalar (n % 4) vs vec")


@pytest.mark.parametrize("accumulate", [0, 1])
def test_sumprod_path_selection_bit_exact(env, accumulate):
    """One term without y (0 + x, or prior + x: one rounding): the two paths agree in bits."""
    base = R.build_sumprod(1024, 1, "none", accumulate, 0, seed=43 + accumulate)
    items = [Item(base), Item(base, {"out": 1}), Item(base, {("x", 0): 1}), Item(_truncated(base, 1023))]
    got = run_sumprod(env, items, "paths")
    assert R.sumprod_exact32(base) is not None
    assert bits_equal(got[1], got[0]) and bits_equal(got[2], got[0]) and bits_equal(got[3], got[0][:1023])


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", [1028, 1029])
def test_sumprod_terms(env, n, accumulate):
    """n_terms in {0, 1, 2, 7, 8} x y {all NULL, all given, NULL for the last term only, NULL for the first term only}
    on the 16-byte path (1028) and the scalar path (1029): 20 items, two argument blocks."""
    run_sumprod(env, [Item(it) for it in R.sumprod_term_items(n, accumulate)], "terms")


@pytest.mark.parametrize("n", [1028, 1029])
def test_sumprod_activation(env, n):
    """RELU, SIGMOID, SIGMOID2 derivatives from deriv_of, whose first values are exact 0, 1, 2 and -0.0."""
    its = R.sumprod_act_items(n)
    for it in its:
        assert bits_equal(it["deriv_of"][:4], np.array(R.ACT_SPECIALS, F32))
    got = run_sumprod(env, [Item(it) for it in its], "activation")
    for it, g in zip(its, got):
        assert g[0] == 0 and g[3] == 0  # act'(0) = act'(-0) = 0 for all three
        if it["act"] == R.ACT_SIGMOID2:
            assert g[2] == 0  # saturated at 2


@pytest.mark.parametrize("n_items", [1, 16, 17, 33])
def test_sumprod_blocks_of_16(env, n_items):
    """Every item has its own data, length and flags: an item of the second or third argument block read from the slot of
    the same number in the first cannot pass."""
    run_sumprod(env, [Item(it) for it in R.sumprod_mixed_items(n_items)], "blocks")


def test_sumprod_empty_block_and_empty_call(env):
    """16 items of n = 0 and then one real item (the `continue` over an empty block), and n_items = 0 with a NULL array."""
    lib = env[0]
    its = [R.build_sumprod(0, i % 3, "all", i % 2, 0, seed=i) for i in range(16)] + [R.build_sumprod(517, 3, "all", 1, 0, 9)]
    run_sumprod(env, [Item(it) for it in its], "blocks")
    ok(lib, lib.mml_sumprod_batch(None, 0, stream()))


def _amax_of(L, lib, pairs, slots):
    """mml_amax_batch over (Arr, slot index) pairs into fresh slots"""
    arr = (L.AmaxDesc * len(pairs))()
    for d, (a, s) in zip(arr, pairs):
        d.x, d.rows, d.ld, d.cols, d.slot = a.ptr, 1, max(a.n, 1), a.n, slots[s].data_ptr()
    ok(lib, lib.mml_amax_batch(arr, len(pairs), stream()))


def test_sumprod_amax_slots(env):
    """Two items share slot 0 (one of them accumulating), one has slot 1, one has none (slot 3 stays 0), one whose output
    holds a NaN has slot 2: every slot equals exactly the largest finite |value| of the bits the items naming it stored,
    and mml_amax_batch over the same outputs gives the same numbers."""
    lib, L, ops = env
    its, slot_of = R.sumprod_amax_items()
    slots = ops.amax_slots(4, dev())
    items = [Item(it, slot=None if s is None else slots[s]) for it, s in zip(its, slot_of)]
    got = run_sumprod(env, items, "amax")
    assert np.isnan(got[4][17]) and int(np.isnan(got[4]).sum()) == 1
    want = [0.0] * 4
    for g, s in zip(got, slot_of):
        if s is not None:
            want[s] = max(want[s], float(np.abs(g[np.isfinite(g)]).max()))
    assert want[0] == float(np.abs(got[1]).max()) > float(np.abs(got[0]).max())  # the accumulated sum it stored
    assert float(np.abs(got[3]).max()) > max(want)  # (the item without a slot holds the largest values of all)
    assert [ops.amax_value(slots[s]) for s in range(4)] == want and want[3] == 0.0
    again = ops.amax_slots(4, dev())
    _amax_of(L, lib, [(it.out, s) for it, s in zip(items, slot_of) if s is not None], again)
    assert [ops.amax_value(again[s]) for s in range(4)] == want


SUMPROD_REJECTIONS = ("n_terms_9", "null_x", "act_with_accumulate", "act_without_deriv_of", "act_4", "act_negative",
                      "null_out")


@pytest.mark.parametrize("bad", [16, 3])
@pytest.mark.parametrize("kind", SUMPROD_REJECTIONS)
def test_sumprod_rejections_write_nothing(env, kind, bad):
    """A malformed item is refused with its index in mml_last_error(), and no output of the call has changed -- items
    0..15 included when the malformed item is number 16 (the whole array is validated before the first launch)."""
    lib, L, ops = env
    its = R.sumprod_mixed_items(17)
    its[bad] = R.build_sumprod(260, 3, "all", 0, 0, seed=77)
    slots = ops.amax_slots(1, dev())
    items = [Item(it, slot=slots[0] if i == 0 else None) for i, it in enumerate(its)]
    arr = descs(L, items)
    d = arr[bad]
    if kind == "n_terms_9":
        d.n_terms = 9
    elif kind == "null_x":
        d.x[1] = None
    elif kind == "act_with_accumulate":
        d.act, d.deriv_of, d.accumulate = R.ACT_RELU, items[bad].xs[0].ptr, 1
    elif kind == "act_without_deriv_of":
        d.act, d.deriv_of = R.ACT_SIGMOID, None
    elif kind == "act_4":
        d.act, d.deriv_of = 4, items[bad].xs[0].ptr
    elif kind == "act_negative":
        d.act, d.deriv_of = -1, items[bad].xs[0].ptr
    else:
        d.out = None
    refused(lib, lib.mml_sumprod_batch(arr, len(items), stream()), f"item {bad}")
    torch.cuda.synchronize()
    for i, it in enumerate(items):
        assert it.out.unchanged(), f"{kind}: the output of item {i} changed"
        assert it.inputs_unchanged()
    assert ops.amax_value(slots[0]) == 0.0


# ---------------------------------------------------------------------------------------------------------------
# 2. mml_gather_fwd_mark and mml_rows_compact
# ---------------------------------------------------------------------------------------------------------------
def byte_map(total):
    """an all-zero map of `total` bytes with 8 * GUARD guard bytes of 0xA5 behind it"""
    m = torch.zeros(total + 8 * GUARD, dtype=torch.uint8, device=dev())
    m[total:] = SENT_BYTE
    return m


def check_byte_map(m, total, want, what):
    host = m.cpu().numpy()
    assert (host[total:] == SENT_BYTE).all(), what + ": written behind the mark map"
    if want is None:
        assert not host[:total].any(), what + ": the mark map is not all zero"
    else:
        assert np.array_equal(host[:total], want), (what, np.flatnonzero(host[:total] != want)[:8])


def gather(env, g, E, Nd, ldo, mark, X=None):
    """mml_gather_fwd (mark = False) or mml_gather_fwd_mark on a sentinel-filled output -> (Buf, marks, status, kernel)"""
    lib, L, ops = env
    vocab, F = g["vocab"], len(g["vocab"])
    X = g["X"] if X is None else X
    B = X.shape[0]
    tabs = [T(t) for t in g["tabs"]]
    Xd = T(X)
    out = Buf(B, F * E + Nd, ldo)
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    total = R.mark_layout(vocab)[1]
    args = (ops._ptr_array(tabs), (L.i64 * F)(*vocab), (L.i32 * F)(*g["col"]), F, E, Xd.data_ptr(), X.shape[1],
            g["dense_col0"], Nd, B, out.ptr, out.ld)
    marks = None
    if mark:
        marks = byte_map(total)
        ok(lib, lib.mml_gather_fwd_mark(*args, marks.data_ptr(), status.data_ptr(), stream()))
    else:
        ok(lib, lib.mml_gather_fwd(*args, status.data_ptr(), stream()))
    kernel = lib.mml_gather_last_kernel().decode()
    torch.cuda.synchronize()
    assert same_bits(Xd.cpu().numpy(), X) and all(same_bits(t.cpu().numpy(), h) for t, h in zip(tabs, g["tabs"]))
    return out, marks, int(status.item()), kernel


def out_ld(width, rem):
    """a leading dimension >= width + 1 with ld % 4 == rem"""
    ld = (width + 4) // 4 * 4 + 4
    return ld + rem


FORM_KERNEL = {"vec4": "gather_vec4_kernel", "scalar_E6": "gather_scalar_kernel", "scalar_ldo": "gather_scalar_kernel"}


@pytest.mark.parametrize("form,E,rem", R.GATHER_FORMS)
@pytest.mark.parametrize("Nd", R.GATHER_ND)
@pytest.mark.parametrize("F", R.GATHER_F)
@pytest.mark.parametrize("B", R.GATHER_B)
def test_gather_fwd_mark(env, B, F, Nd, form, E, rem):
    """The output (padding included) has the bits mml_gather_fwd writes and those of the numpy gather; byte
    markbase[f] + r is 1 exactly for the rows some sample of field f names, every other byte of the map -- the tails
    between V_f and 32 ceil(V_f / 32), the guard bytes -- is untouched; the kernel that ran is the one the form selects."""
    shift = R.GATHER_B.index(B)
    g = R.build_gather(B, F, Nd, E, shift, seed=B + 7 * F + Nd)
    ldo = out_ld(F * E + Nd, rem)
    plain, _, st0, k0 = gather(env, g, E, Nd, ldo, mark=False)
    marked, marks, st1, k1 = gather(env, g, E, Nd, ldo, mark=True)
    what = f"mml_gather_fwd_mark {form} B={B} F={F} Nd={Nd}"
    assert k0 == k1 == FORM_KERNEL[form], (k0, k1)
    assert st0 == 0 and st1 == 0
    got = marked.get(what)
    assert np.array_equal(marked.words(), plain.words()), what + ": not the bits of mml_gather_fwd"
    assert same_bits(got, R.ref_gather(g["tabs"], g["rows"], g["X"], g["dense_col0"], Nd)), what
    check_byte_map(marks, R.mark_layout(g["vocab"])[1], R.ref_mark_map(g["rows"], g["vocab"]), what)


@pytest.mark.parametrize("form,E,rem", R.GATHER_FORMS)
def test_gather_fwd_mark_out_of_range(env, form, E, rem):
    """One negative index and one >= V: status bits 1 and 2, the clamped rows (0 and V - 1) gathered as by mml_gather_fwd
    and marked -- no other sample names them."""
    B, F, Nd = 257, 3, 5
    g = R.build_gather(B, F, Nd, E, 2, seed=11)  # vocab (32, 33, 1000)
    vocab = g["vocab"]
    rng = np.random.default_rng(12)
    rows = np.stack([rng.integers(1, v - 1, B) for v in vocab], 1)
    X = g["X"].copy()
    for f in range(F):
        X[:, g["col"][f]] = rows[:, f].astype(F32)
    X[5, g["col"][0]] = -3.0
    X[9, g["col"][2]] = float(vocab[2] + 5)
    idx = rows.copy()
    idx[5, 0], idx[9, 2] = -3, vocab[2] + 5
    clamped, status = R.clamp_rows(idx, vocab)
    assert status == 3 and clamped[5, 0] == 0 and clamped[9, 2] == vocab[2] - 1
    ldo = out_ld(F * E + Nd, rem)
    plain, _, st0, _ = gather(env, g, E, Nd, ldo, mark=False, X=X)
    marked, marks, st1, k1 = gather(env, g, E, Nd, ldo, mark=True, X=X)
    assert (st0, st1) == (3, 3) and k1 == FORM_KERNEL[form]
    assert np.array_equal(marked.words(), plain.words())
    assert same_bits(marked.get(form), R.ref_gather(g["tabs"], clamped, X, g["dense_col0"], Nd))
    want = R.ref_mark_map(clamped, vocab)
    base = R.mark_layout(vocab)[0]
    assert want[base[0]] == 1 and want[base[2] + vocab[2] - 1] == 1 and int(want.sum()) == sum(
        len(np.unique(clamped[:, f])) for f in range(F))
    check_byte_map(marks, R.mark_layout(vocab)[1], want, "out of range " + form)


def test_gather_fwd_mark_ignores_the_lds_variant(env, monkeypatch):
    """MMLREC_GATHER_LDS=4 sends mml_gather_fwd to gather_lds_kernel, which marks nothing: the marking call must still
    run gather_vec4_kernel and mark."""
    B, F, Nd, E = 257, 3, 5, 8
    g = R.build_gather(B, F, Nd, E, 1, seed=21)
    ldo = out_ld(F * E + Nd, 0)
    monkeypatch.setenv("MMLREC_GATHER_LDS", "4")
    plain, _, _, k0 = gather(env, g, E, Nd, ldo, mark=False)
    marked, marks, st, k1 = gather(env, g, E, Nd, ldo, mark=True)
    assert k0 == "gather_lds_kernel" and k1 == "gather_vec4_kernel" and st == 0
    assert np.array_equal(marked.words(), plain.words())
    check_byte_map(marks, R.mark_layout(g["vocab"])[1], R.ref_mark_map(g["rows"], g["vocab"]), "lds")


class Compact:
    """Device state of mml_rows_compact: `seen` bitmaps (GUARD sentinel words behind each), the mark map, the list of
    `cap` entries (GUARD sentinel words behind it) and the counter."""

    def __init__(self, env, vocab, old, cap):
        self.lib, self.L, self.ops = env
        self.vocab, self.cap, self.F = [int(v) for v in vocab], int(cap), len(vocab)
        self.rb = R.row_base(vocab)
        self.base, self.total = R.mark_layout(vocab)
        self.seen = []
        for o, v in zip(old, self.vocab):
            w = np.concatenate([o if o.dtype == np.uint32 else R.rows_to_bitmap(o, v),
                                np.full(GUARD, np.uint32(0xA5A5A5A5), np.uint32)])
            self.seen.append(T(w.view(np.int32)))
        self.marks = byte_map(self.total)
        self.touched = torch.full((self.cap + GUARD,), SENT_I32, dtype=torch.int32, device=dev())
        self.count = torch.full((1 + GUARD,), SENT_I32, dtype=torch.int32, device=dev())

    def mark(self, rows):
        """sets the mark bytes on the device from an index tensor"""
        pos = np.concatenate([np.asarray(r, dtype=np.int64) + b for r, b in zip(rows, self.base)])
        self.marks[T(pos)] = 1

    def run(self, use_marks=True):
        L = self.L
        ok(self.lib, self.lib.mml_rows_compact(self.ops._ptr_array(self.seen), (L.i64 * self.F)(*self.vocab),
                                               (L.i64 * (self.F + 1))(*self.rb), self.F, self.touched.data_ptr(),
                                               self.count.data_ptr(), self.cap,
                                               self.marks.data_ptr() if use_marks else None, stream()))
        torch.cuda.synchronize()

    def seen_words(self):
        out = []
        for s, v in zip(self.seen, self.vocab):
            w = s.cpu().numpy().view(np.uint32)
            assert (w[R.words_of(v):] == np.uint32(0xA5A5A5A5)).all(), "written behind a bitmap"
            out.append(w[:R.words_of(v)].copy())
        return out

    def check(self, ids, after, what):
        """count exact, list = the reference set without duplicates (or, under a short cap, `cap` distinct members of
        it), nothing else in the list buffer written, bitmaps = after, mark map all zero"""
        cnt = self.count.cpu().numpy()
        assert (cnt[1:] == SENT_I32).all(), what + ": written behind the counter"
        assert int(cnt[0]) == len(ids), (what, int(cnt[0]), len(ids))
        lst = self.touched.cpu().numpy()
        k = min(len(ids), self.cap)
        assert (lst[k:] == SENT_I32).all(), what + ": the list was written behind its entries"
        got = np.sort(lst[:k].astype(np.int64))
        assert len(np.unique(got)) == k, what + ": duplicates in the list"
        if k == len(ids):
            assert np.array_equal(got, ids), what
        else:
            assert np.isin(got, ids).all(), what + ": an entry outside the reference set"
        for f, (w, a) in enumerate(zip(self.seen_words(), after)):
            assert np.array_equal(w, a), (what, f, np.flatnonzero(w != a)[:8])
        assert not bool(self.marks[:self.total].any()), what + ": the mark map is not all zero"
        assert bool((self.marks[self.total:] == SENT_BYTE).all()), what + ": written behind the mark map"


COMPACT_CASES = {
    "F1_V1": [1], "V31": [31], "V32": [32], "V33": [33], "one_workgroup": [32 * 1024], "second_workgroup": [32 * 1024 + 1],
    "max_fields": [(1, 31, 32, 33, 1000, 32 * 1024 + 1, 70000, 5000)[f % 8] for f in range(R.MAX_FIELDS)],
}


@pytest.mark.parametrize("case", list(COMPACT_CASES))
def test_rows_compact(env, case):
    """Old `seen` bits and new marks in words of all four kinds (only old, only new, both, neither).  First call: list,
    count, seen = old | marks, marks cleared.  Second call without new marks: the same set from the bitmaps, the count
    not doubled.  Third call with row_marks = NULL: the list is the bits, the bitmaps are unchanged."""
    vocab = COMPACT_CASES[case]
    old, new = R.build_compact(vocab, seed=len(vocab) + vocab[0])
    if max(vocab) >= 1000:
        f = int(np.argmax(vocab))
        assert min(R.word_census(old[f], new[f], vocab[f])) >= 1
    seen0 = [R.rows_to_bitmap(o, v) for o, v in zip(old, vocab)]
    ids, after = R.ref_compact(seen0, new, vocab)
    assert np.array_equal(ids, np.concatenate([np.union1d(o, m) + b for o, m, b in zip(old, new, R.row_base(vocab))]))
    c = Compact(env, vocab, old, cap=len(ids) + 3)
    c.mark(new)
    c.run()
    c.check(ids, after, case + " first call")
    c.touched.fill_(SENT_I32)
    c.run()
    c.check(ids, after, case + " second call")
    c.touched.fill_(SENT_I32)
    c.run(use_marks=False)
    c.check(ids, after, case + " without a mark map")


def test_rows_compact_without_marks_ignores_the_map(env):
    """row_marks = NULL on fresh state: the list is the bitmaps' bits (a set mark byte is not this call's business)."""
    vocab = [1000, 33]
    old, new = R.build_compact(vocab, seed=3)
    ids, after = R.ref_compact([R.rows_to_bitmap(o, v) for o, v in zip(old, vocab)], None, vocab)
    c = Compact(env, vocab, old, cap=len(ids))
    c.run(use_marks=False)
    c.check(ids, after, "no map")


@pytest.mark.parametrize("cap_of", ["one", "half", "count_minus_one", "count"])
def test_rows_compact_short_list(env, cap_of):
    """touched_cap below the count: *touched_count still reports the full number, exactly `cap` entries are written, they
    are distinct members of the reference set, and nothing behind touched[cap) is written."""
    vocab = [1000, 33, 32 * 1024 + 1]
    old, new = R.build_compact(vocab, seed=8)
    ids, after = R.ref_compact([R.rows_to_bitmap(o, v) for o, v in zip(old, vocab)], new, vocab)
    cap = dict(one=1, half=len(ids) // 2, count_minus_one=len(ids) - 1, count=len(ids))[cap_of]
    c = Compact(env, vocab, old, cap=cap)
    c.mark(new)
    c.run()
    c.check(ids, after, f"cap {cap} of {len(ids)}")
    assert (c.touched[:cap].cpu().numpy() != SENT_I32).all()


def test_rows_compact_second_trip_of_the_workgroup_loop(env):
    """A field gets at most 1024 workgroups of 1024 words: V = 2^25 + 100 000 rows (33.7 MB of marks, set on the device)
    sends the words of rows >= 2^25 through a second trip.  No shipped workload reaches it (largest table: 12.49 M rows)."""
    V = 2 ** 25 + 100000
    assert R.words_of(V) > 1024 * 1024
    rng = np.random.default_rng(5)
    new = np.unique(np.concatenate([rng.integers(0, V, 50000), [0, 2 ** 25 - 1, 2 ** 25, V - 1]]))
    old = np.unique(np.concatenate([rng.integers(2 ** 25 - 200000, 2 ** 25, 500), rng.integers(2 ** 25, V, 500),
                                    [2 ** 25 - 2, 2 ** 25 + 1, 1]]))  # (2^25 - 2, 2^25 + 1: words with a mark as well)
    seen0 = R.rows_to_bitmap(old, V)
    ids, after = R.ref_compact([seen0], [new], [V])
    assert len(ids) == len(np.union1d(old, new)) and (ids >= 2 ** 25).sum() > 600
    c = Compact(env, [V], [seen0], cap=len(ids) + 5)
    c.mark([new])
    c.run()
    c.check(ids, after, "second trip")


@pytest.mark.parametrize("B,F", [(4096, R.MAX_FIELDS), (257, 3)])
def test_gather_mark_then_compact_is_index_unique(env, B, F):
    """mml_gather_fwd_mark + mml_rows_compact yields the set mml_index_unique (with row_marks) builds from the same X,
    and np.unique's."""
    lib, L, ops = env
    E, Nd = 8, 5
    g = R.build_gather(B, F, Nd, E, 1, seed=B + F)
    vocab = g["vocab"]
    rb = R.row_base(vocab)
    want = np.concatenate([np.unique(g["rows"][:, f]) + rb[f] for f in range(F)])
    zero = [np.zeros(0, np.int64)] * F
    a = Compact(env, vocab, zero, cap=B * F)
    _, marks, _, _ = gather(env, g, E, Nd, out_ld(F * E + Nd, 0), mark=True)
    a.marks = marks
    a.run()
    a.check(want, R.ref_compact([R.rows_to_bitmap([], v) for v in vocab], [g["rows"][:, f] for f in range(F)], vocab)[1],
            "gather + compact")
    b = Compact(env, vocab, zero, cap=B * F)
    Xd = T(g["X"])
    ok(lib, lib.mml_index_unique((L.i64 * F)(*vocab), (L.i32 * F)(*g["col"]), F, E, Xd.data_ptr(), g["X"].shape[1], B,
                                 ops._ptr_array(b.seen), (L.i64 * (F + 1))(*rb), b.touched.data_ptr(),
                                 b.count.data_ptr(), b.cap, b.marks.data_ptr(), None, stream()))
    torch.cuda.synchronize()
    b.check(want, a.seen_words(), "index_unique")


# ---------------------------------------------------------------------------------------------------------------
# 3. mml_shard_rows
# ---------------------------------------------------------------------------------------------------------------
def _table(V, E, seed):
    return np.random.default_rng(seed).standard_normal((V, E)).astype(F32)


@pytest.mark.parametrize("E", R.SHARD_E)
@pytest.mark.parametrize("V", R.SHARD_V)
@pytest.mark.parametrize("world", R.SHARD_WORLDS)
def test_shard_rows_to_shard(lib, world, V, E):
    """shard = table[first::world], zero rows up to rows_local = ceil(V / world) (and, for rank 0, three rows more),
    bit-equal; nothing behind the shard, the table untouched -- for every first < world."""
    table = _table(V, E, V + E)
    tb = Buf(V, E, data=table)
    for first in range(world):
        for rows_local in ((V + world - 1) // world,) + (((V + world - 1) // world + 3,) if first == 0 else ()):
            sh = Buf(rows_local, E)
            ok(lib, lib.mml_shard_rows(tb.ptr, V, sh.ptr, rows_local, E, world, first, 0, stream()))
            assert same_bits(sh.get("shard"), R.ref_shard(table, world, first, rows_local)), (first, rows_local)
    assert tb.unchanged()


@pytest.mark.parametrize("E", R.SHARD_E)
@pytest.mark.parametrize("V", R.SHARD_V)
@pytest.mark.parametrize("world", R.SHARD_WORLDS)
def test_shard_rows_to_table(lib, world, V, E):
    """Only rows first, first + world, ... < V change; every other row and the guard row keep the sentinel; the shards
    of all ranks written back in turn rebuild the table bit for bit."""
    table = _table(V, E, V + E)
    tb = Buf(V, E)
    state = tb.before[:V].view(F32).copy()
    rows_local = (V + world - 1) // world
    for first in range(world):
        sh = Buf(rows_local, E, data=R.ref_shard(table, world, first, rows_local))
        ok(lib, lib.mml_shard_rows(tb.ptr, V, sh.ptr, rows_local, E, world, first, 1, stream()))
        state = R.ref_unshard(state, sh.before[:rows_local].view(F32), world, first)
        assert same_bits(tb.get("table"), state), first
        assert sh.unchanged()
    assert same_bits(state, table)


@pytest.mark.parametrize("to_table", [0, 1])
def test_shard_rows_beyond_the_grid_cap(lib, to_table):
    """70 000 x 16 = 1.12 M elements > 4096 workgroups x 256 threads: the grid-stride loop runs a second trip."""
    V, E = 70000, 16
    assert V * E > 4096 * 256
    table = _table(V, E, 1)
    if to_table:
        tb, sh = Buf(V, E), Buf(V, E, data=table)
        ok(lib, lib.mml_shard_rows(tb.ptr, V, sh.ptr, V, E, 1, 0, 1, stream()))
        assert same_bits(tb.get("table"), table) and sh.unchanged()
    else:
        tb, sh = Buf(V, E, data=table), Buf(V, E)
        ok(lib, lib.mml_shard_rows(tb.ptr, V, sh.ptr, V, E, 1, 0, 0, stream()))
        assert same_bits(sh.get("shard"), table) and tb.unchanged()


@pytest.mark.parametrize("world", [1, 3, 8])
def test_shard_rows_layout_of_row_sharding(env, world):
    """first, rows_local and keybase from parallel.RowSharding for three fields: the flat shard built field by field on
    the device is the one the host arithmetic of tests/test_parallel_cpu.py builds."""
    lib = env[0]
    from mmlrec_amd.parallel import RowSharding
    vocab, E = [1000, 7, 64], 4
    tabs = [_table(v, E, v) for v in vocab]
    tbs = [Buf(v, E, data=t) for v, t in zip(vocab, tabs)]
    for rank in range(world):
        sh = RowSharding(vocab, E, world, rank)
        flat = Buf(sh.R, E)
        want = flat.before[:sh.R].view(F32).copy()
        for f, v in enumerate(vocab):
            ok(lib, lib.mml_shard_rows(tbs[f].ptr, v, flat.ptr + 4 * E * sh.keybase[f], sh.rows_local[f], E, world,
                                       sh.first(f), 0, stream()))
            rows = np.arange(sh.first(f), v, world)
            assert len(rows) == sh.owned_rows(f)
            want[sh.keybase[f]:sh.keybase[f + 1]] = 0
            want[sh.keybase[f]:sh.keybase[f] + len(rows)] = tabs[f][rows]
        assert same_bits(flat.get("flat shard"), want), rank


@pytest.mark.parametrize("kind", ["first_is_world", "V_zero", "null_table", "null_shard"])
@pytest.mark.parametrize("to_table", [0, 1])
def test_shard_rows_rejections_write_nothing(lib, kind, to_table):
    V, E, world = 7, 4, 3
    tb, sh = Buf(V, E, data=_table(V, E, 1)), Buf(3, E, data=_table(3, E, 2))
    args = dict(table=tb.ptr, V=V, shard=sh.ptr, first=1)
    args.update({"first_is_world": dict(first=world), "V_zero": dict(V=0), "null_table": dict(table=None),
                 "null_shard": dict(shard=None)}[kind])
    refused(lib, lib.mml_shard_rows(args["table"], args["V"], args["shard"], 3, E, world, args["first"], to_table, stream()),
            "mml_shard_rows")
    torch.cuda.synchronize()
    assert tb.unchanged() and sh.unchanged()


# ---------------------------------------------------------------------------------------------------------------
# 4. the thin neighbours in csrc/ew.hip
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.EW_LENGTHS)
def test_ew_mul_and_add_n(env, n):
    """mml_ew_mul: the float32 product; mml_ew_add_n of 1, 2, 16 inputs: the in-order float32 sum 0 + in[0] + ...;
    n_in = 17 and n_in = 0 are refused (MML_REQUIRE n_in in [1, 16]) and write nothing."""
    lib, L, ops = env
    w = R.build_ew(n, n)
    a, b, out = Arr(n, w["a"]), Arr(n, w["b"]), Arr(n)
    ok(lib, lib.mml_ew_mul(a.ptr, b.ptr, out.ptr, n, stream()))
    assert bits_equal(out.get("ew_mul"), w["a"] * w["b"]) and a.unchanged() and b.unchanged()
    rng = np.random.default_rng(n + 1)
    host = [rng.standard_normal(n).astype(F32) for _ in range(17)]
    ins = [Arr(n, h) for h in host]
    for n_in in (1, 2, 16):
        out = Arr(n)
        ok(lib, lib.mml_ew_add_n(ops._ptr_array([i.t for i in ins[:n_in]]), n_in, out.ptr, n, stream()))
        assert bits_equal(out.get("ew_add_n"), R.f32_add_n(host[:n_in])), n_in
    for n_in in (17, 0):
        out = Arr(n)
        refused(lib, lib.mml_ew_add_n(ops._ptr_array([i.t for i in ins]), n_in, out.ptr, n, stream()), "mml_ew_add_n")
        torch.cuda.synchronize()
        assert out.unchanged()
    assert all(i.unchanged() for i in ins)


@pytest.mark.parametrize("want", ["da", "db", "both"])
@pytest.mark.parametrize("n", R.EW_LENGTHS)
def test_ew_mul_bwd(lib, n, want):
    """da (+)= dout b, db (+)= dout a with da NULL, db NULL, both: bit-equal to the float32 product without
    accumulation, within 2 x 2^-24 sum|terms| with it (one product, one add)."""
    w = R.build_ew(n, 3 * n)
    d, a, b = Arr(n, w["d"]), Arr(n, w["a"]), Arr(n, w["b"])
    for acc in (0, 1):
        da = Arr(n, w["pa"]) if want != "db" else None
        db = Arr(n, w["pb"]) if want != "da" else None
        ok(lib, lib.mml_ew_mul_bwd(d.ptr, a.ptr, b.ptr, da.ptr if da else None, db.ptr if db else None, acc, acc, n,
                                   stream()))
        rda, sa, rdb, sb = R.ref64_mul_bwd(w["d"], w["a"], w["b"], w["pa"] if acc else None, w["pb"] if acc else None)
        for got, ref, s, f32 in ((da, rda, sa, w["d"] * w["b"]), (db, rdb, sb, w["d"] * w["a"])):
            if got is None:
                continue
            g = got.get("ew_mul_bwd")
            if acc:
                assert_close_terms(g, ref, s, 2 * R.TWO24, "mml_ew_mul_bwd: accumulate")
            else:
                assert bits_equal(g, f32)
    assert d.unchanged() and a.unchanged() and b.unchanged()


@pytest.mark.parametrize("act_a,act_b", [(R.ACT_RELU, R.ACT_SIGMOID2), (R.ACT_SIGMOID, R.ACT_RELU),
                                          (R.ACT_SIGMOID2, R.ACT_SIGMOID), (R.ACT_NONE, R.ACT_SIGMOID2)])
@pytest.mark.parametrize("n", R.EW_LENGTHS)
def test_ew_mul_bwd_act_and_act_bwd(lib, n, act_a, act_b):
    """The folded derivatives of all three activations, operands that begin with the saturated outputs 0, 1, 2, -0:
    4 x 2^-24 sum|terms| (dout b, at most two roundings in act', the product)."""
    rng = np.random.default_rng(n + act_a)
    w = R.build_ew(n, n + 5)
    ah = R.act_outputs(act_a, n, rng) if act_a else w["a"]
    bh = R.act_outputs(act_b, n, rng)
    d, a, b, da, db = Arr(n, w["d"]), Arr(n, ah), Arr(n, bh), Arr(n), Arr(n)
    ok(lib, lib.mml_ew_mul_bwd_act(d.ptr, a.ptr, b.ptr, da.ptr, db.ptr, 0, 0, n, act_a, act_b, stream()))
    rda, sa, rdb, sb = R.ref64_mul_bwd(w["d"], ah, bh, None, None, act_a, act_b)
    assert_close_terms(da.get("da"), rda, sa, 4 * R.TWO24, "mml_ew_mul_bwd_act: da")
    assert_close_terms(db.get("db"), rdb, sb, 4 * R.TWO24, "mml_ew_mul_bwd_act: db")
    dst = Arr(n)
    ok(lib, lib.mml_act_bwd(b.ptr, d.ptr, dst.ptr, n, act_b, stream()))
    ref, s = R.ref64_act_bwd(bh, w["d"], act_b)
    got = dst.get("act_bwd")
    assert_close_terms(got, ref, s, 4 * R.TWO24, "mml_act_bwd: dst")
    assert got[0] == 0 and (n < 4 or got[3] == 0) and (n < 3 or act_b != R.ACT_SIGMOID2 or got[2] == 0)
    assert d.unchanged() and a.unchanged() and b.unchanged()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("cols", [1, 5, 64])
def test_copy2d(lib, cols, accumulate):
    """dst[r, c] (+)= src[r, c] with lds != ldd: bit-equal to float32 numpy; padding columns and the row behind keep the
    sentinel, the source keeps its bits."""
    rows = 37
    rng = np.random.default_rng(cols)
    src = Buf(rows, cols, cols + 3, rng.standard_normal((rows, cols)).astype(F32))
    dst = Buf(rows, cols, cols + 2, rng.standard_normal((rows, cols)).astype(F32))
    ok(lib, lib.mml_copy2d(src.ptr, src.ld, dst.ptr, dst.ld, rows, cols, accumulate, stream()))
    want = R.f32_copy2d(src.before.view(F32), dst.before.view(F32), rows, cols, accumulate)
    assert np.array_equal(dst.words(), want.view(np.uint32)) and src.unchanged()
    dst.get("copy2d")
