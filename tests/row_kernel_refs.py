"""Host references of the kernel tests for mml_sumprod_batch, mml_gather_fwd_mark, mml_rows_compact, mml_shard_rows and
the small elementwise entry points of csrc/ew.hip (tests/test_row_kernel_refs_cpu.py proves them on the host,
tests/test_row_kernels_gpu.py uses them on the device).  numpy only: no torch, no GPU, no fixtures.

  ref64_*    float64 statements of the contracts of include/mmlrec.h; a sum comes with the per-element sum of the
             absolute values of its terms ("sumabs"), which is what a tolerance multiplies.
  f32_*      float32 numpy restatements used where the device arithmetic has at most one rounding (bit equality).
  model32_sumprod   the float32 chain of sumprod_batch_kernel with named mutations: the CPU file proves that tolerance +
             inputs notice each of them; never a reference for the GPU.
  mark / bitmap / shard helpers   the layouts in plain integer arithmetic.
  build_* / *_CASES   seeded inputs and the case lists both test files share.
"""
import numpy as np

from model_kernel_refs import F32, F64, RATIOS, assert_close_terms, bits_equal  # noqa: F401  (re-exported)

TWO24 = 2.0 ** -24
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SIGMOID2 = 0, 1, 2, 3
ACTS = (ACT_RELU, ACT_SIGMOID, ACT_SIGMOID2)
MAX_FIELDS, SUMPROD_TERMS, SUMPROD_BATCH = 64, 8, 16
ACT_SPECIALS = (0.0, 1.0, 2.0, -0.0)  # exact 0 / 1 / 2 (sigmoid2 saturated) / negative zero, first in every deriv_of


# ---------------------------------------------------------------------------------------------------------------
# activation derivative from the activation's OUTPUT
# ---------------------------------------------------------------------------------------------------------------
def act_deriv64(o, act):
    o = np.asarray(o).astype(F64)
    if act == ACT_RELU:
        return (o > 0).astype(F64)
    if act == ACT_SIGMOID:
        return o * (1.0 - o)
    if act == ACT_SIGMOID2:
        return o * (1.0 - 0.5 * o)
    assert act == ACT_NONE
    return np.ones_like(o)


def act_deriv32(o, act, mutate=None):
    o = np.asarray(o, dtype=F32)
    if act == ACT_SIGMOID2 and mutate == "sigmoid_for_sigmoid2":
        act = ACT_SIGMOID
    if act == ACT_RELU:
        return (o > 0).astype(F32)
    if act == ACT_SIGMOID:
        return (o * (F32(1) - o).astype(F32)).astype(F32)
    if act == ACT_SIGMOID2:
        return (o * (F32(1) - (F32(0.5) * o).astype(F32)).astype(F32)).astype(F32)
    return np.ones_like(o)


def act_outputs(act, n, rng):
    """n float32 outputs of the activation (relu / sigmoid / 2 sigmoid of 2 N(0, 1)); ACT_SPECIALS come first."""
    z = 2.0 * rng.standard_normal(n)
    o = np.maximum(z, 0.0) if act == ACT_RELU else (1.0 if act == ACT_SIGMOID else 2.0) / (1.0 + np.exp(-z))
    o = o.astype(F32)
    k = min(n, len(ACT_SPECIALS))
    o[:k] = np.array(ACT_SPECIALS[:k], F32)
    return o


# ---------------------------------------------------------------------------------------------------------------
# mml_sumprod_batch: out[i] (+)= sum_k x_k[i] * (y_k ? y_k[i] : 1), times act'(deriv_of[i]) when folded
# ---------------------------------------------------------------------------------------------------------------
Y_PATTERNS = ("none", "all", "last_null", "first_null")


def y_pattern(pat, n_terms):
    """which terms carry a y: none, all, all but the last, all but the first"""
    has = [pat != "none"] * n_terms
    if n_terms and pat == "last_null":
        has[-1] = False
    if n_terms and pat == "first_null":
        has[0] = False
    return has


def build_sumprod(n, n_terms, ypat, accumulate, act, seed):
    """One item: xs, ys (None = NULL), the prior (what `out` holds before when accumulating), deriv_of (None without act)."""
    assert not (act and accumulate)
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal(n).astype(F32) for _ in range(n_terms)]
    ys = [rng.standard_normal(n).astype(F32) if h else None for h in y_pattern(ypat, n_terms)]
    prior = rng.standard_normal(n).astype(F32)
    return dict(n=n, n_terms=n_terms, ypat=ypat, accumulate=int(accumulate), act=act, xs=xs, ys=ys, prior=prior,
                deriv_of=act_outputs(act, n, rng) if act else None)


def ref64_sumprod(xs, ys, prior=None, deriv_of=None, act=ACT_NONE, n=None):
    """Returns (out, sumabs): sumabs = (|prior| + sum_k |x_k y_k|) |act'|.  `prior` = None: no accumulation."""
    n = len(xs[0]) if xs else (len(prior) if prior is not None else n)
    out, sa = np.zeros(n, F64), np.zeros(n, F64)
    if prior is not None:
        out, sa = out + prior.astype(F64), sa + np.abs(prior.astype(F64))
    for x, y in zip(xs, ys):
        t = x.astype(F64) * (y.astype(F64) if y is not None else 1.0)
        out, sa = out + t, sa + np.abs(t)
    if act != ACT_NONE:
        d = act_deriv64(deriv_of, act)
        out, sa = out * d, sa * np.abs(d)
    return out, sa


def ref64_sumprod_item(it):
    return ref64_sumprod(it["xs"], it["ys"], it["prior"] if it["accumulate"] else None, it["deriv_of"], it["act"], it["n"])


def model32_sumprod(it, mutate=None):
    """float32 restatement (mul, add, one rounding each; the kernel may contract them into an fma, which the tolerance
    covers).  Mutations: last_y_ignored, prior_dropped, sigmoid_for_sigmoid2."""
    n = it["n"]
    s = it["prior"].copy() if it["accumulate"] and mutate != "prior_dropped" else np.zeros(n, F32)
    for k, (x, y) in enumerate(zip(it["xs"], it["ys"])):
        if y is not None and mutate == "last_y_ignored" and k == it["n_terms"] - 1:
            y = None
        s = (s + ((x * y).astype(F32) if y is not None else x)).astype(F32)
    if it["act"] != ACT_NONE:
        s = (s * act_deriv32(it["deriv_of"], it["act"], mutate)).astype(F32)
    return s


def sumprod_tol(n_terms):
    """(n_terms + 4) 2^-24: n_terms roundings of the fma or mul + add chain, one for the accumulated prior, three for
    y (1 - 0.5 y) and the final product.  (Un-contracted, the products' own roundings are 2^-24 |x_k y_k| each, together
    one more 2^-24 sumabs: the prior's unit covers them, its own add being one of the n_terms.)"""
    return (n_terms + 4) * TWO24


def sumprod_mutation_applies(it, mutate):
    if it["n"] == 0:
        return False
    if mutate == "last_y_ignored":
        return it["n_terms"] > 0 and it["ys"][-1] is not None
    if mutate == "prior_dropped":
        return bool(it["accumulate"])
    if mutate == "sigmoid_for_sigmoid2":
        return it["act"] == ACT_SIGMOID2 and it["n_terms"] > 0
    raise ValueError(mutate)


SUMPROD_MUTATIONS = ("last_y_ignored", "prior_dropped", "sigmoid_for_sigmoid2")


def sumprod_exact32(it):
    """The float32 result where the arithmetic has a single rounding or none, else None: no term (zeros, or the prior's
    bits), one term (0 + x, 0 + x y, prior + x)."""
    if it["act"] != ACT_NONE or it["n_terms"] > 1:
        return None
    if it["n_terms"] == 0:
        return it["prior"].copy() if it["accumulate"] else np.zeros(it["n"], F32)
    x, y = it["xs"][0], it["ys"][0]
    if it["accumulate"]:
        return (it["prior"] + x).astype(F32) if y is None else None  # (prior + x y: two roundings un-contracted)
    return (F32(0) + (x if y is None else (x * y).astype(F32))).astype(F32)


SUMPROD_LENGTHS = (0, 1, 3, 4, 5, 1023, 1024, 4100)
SUMPROD_SCALAR_TWO_TRIPS = 33001   # n % 4 = 1: scalar path, 33 001 > 128 x 256 threads of a capped 16-item block
SUMPROD_VEC_TWO_TRIPS = 140004     # aligned: n / 4 = 35 001 pieces > 128 x 256
SUMPROD_NTERMS = (0, 1, 2, 7, 8)


def sumprod_length_items(accumulate):
    """one argument block of 16: every length of SUMPROD_LENGTHS, the two items that need a second grid-stride trip under
    the block's cap of max(2048 / 16, 64) = 128 workgroups, and six more (with a folded sigmoid2' when not accumulating)"""
    act = ACT_NONE if accumulate else ACT_SIGMOID2
    its = [build_sumprod(n, 2, "last_null", accumulate, ACT_NONE, seed=n + accumulate) for n in SUMPROD_LENGTHS]
    its += [build_sumprod(SUMPROD_SCALAR_TWO_TRIPS, 2, "last_null", accumulate, ACT_NONE, seed=1 + accumulate),
            build_sumprod(SUMPROD_VEC_TWO_TRIPS, 2, "first_null", accumulate, ACT_NONE, seed=2 + accumulate)]
    its += [build_sumprod(n, 3, "all", accumulate, act, seed=3 * n + accumulate) for n in (3, 4, 5, 1023, 1024, 4100)]
    assert len(its) == SUMPROD_BATCH
    return its


def sumprod_term_items(n, accumulate):
    """every n_terms x y pattern at one length: 20 items = two argument blocks"""
    return [build_sumprod(n, nt, pat, accumulate, ACT_NONE, seed=1000 * n + 10 * nt + i + accumulate)
            for nt in SUMPROD_NTERMS for i, pat in enumerate(Y_PATTERNS)]


def sumprod_act_items(n):
    return [build_sumprod(n, nt, pat, 0, act, seed=77 * n + 10 * act + nt)
            for act in ACTS for nt, pat in ((1, "none"), (3, "last_null"), (8, "all"))]


def sumprod_path_base(mode):
    """the item every path-selection variant shares: three terms, a y on each (the last too); mode: act / accumulate / plain"""
    act, acc = (ACT_SIGMOID2, 0) if mode == "act" else (ACT_NONE, int(mode == "accumulate"))
    return build_sumprod(1024, 3, "all", acc, act, seed=41 + act + acc)


def sumprod_amax_items():
    """two items for slot 0 (the second accumulates and holds the slot's maximum), one for slot 1, one without a slot
    (the largest values of all), one for slot 2 whose output holds a single NaN"""
    its = [build_sumprod(1028, 2, "all", 0, ACT_NONE, seed=1), build_sumprod(517, 3, "last_null", 1, ACT_NONE, seed=2),
           build_sumprod(300, 1, "none", 0, ACT_SIGMOID2, seed=3), build_sumprod(64, 2, "all", 0, ACT_NONE, seed=4),
           build_sumprod(260, 2, "last_null", 0, ACT_NONE, seed=5)]
    its[0]["xs"][0] *= F32(0.01)
    its[0]["xs"][1] *= F32(0.01)
    its[3]["xs"][0] *= F32(100)
    its[4]["xs"][1][17] = np.nan
    return its, [0, 0, 1, None, 2]


def sumprod_mixed_items(n_items):
    """n_items items with different data, lengths and flags each (an item read from another slot cannot pass)"""
    lens = (5, 1024, 37, 260, 1, 1023, 4100, 64, 3, 516, 129, 2048, 7, 4, 700, 96, 333)
    items = []
    for i in range(n_items):
        act = (ACT_NONE, ACT_RELU, ACT_NONE, ACT_SIGMOID2, ACT_NONE, ACT_SIGMOID)[i % 6]
        items.append(build_sumprod(lens[i % len(lens)] + 4 * (i // len(lens)), (i * 2 + 1) % 9, Y_PATTERNS[(i + 1) % 4],
                                   0 if act else (i // 2) % 2, act, seed=5000 + i))
    return items


# ---------------------------------------------------------------------------------------------------------------
# the other elementwise entry points of csrc/ew.hip
# ---------------------------------------------------------------------------------------------------------------
EW_LENGTHS = (1, 255, 257, 70001)


def build_ew(n, seed):
    rng = np.random.default_rng(seed)
    return dict(a=rng.standard_normal(n).astype(F32), b=rng.standard_normal(n).astype(F32),
                d=rng.standard_normal(n).astype(F32), pa=rng.standard_normal(n).astype(F32),
                pb=rng.standard_normal(n).astype(F32))


def f32_add_n(ins):
    """0 + in[0] + in[1] + ... in order, every add rounded to float32"""
    s = np.zeros_like(ins[0])
    for x in ins:
        s = (s + x).astype(F32)
    return s


def ref64_mul_bwd(d, a, b, prior_a=None, prior_b=None, act_a=ACT_NONE, act_b=ACT_NONE):
    """da (+)= d b act_a'(a), db (+)= d a act_b'(b).  Returns da, da_sumabs, db, db_sumabs."""
    d, a64, b64 = d.astype(F64), a.astype(F64), b.astype(F64)
    da, db = d * b64 * act_deriv64(a, act_a), d * a64 * act_deriv64(b, act_b)
    sa, sb = np.abs(da), np.abs(db)
    if prior_a is not None:
        da, sa = da + prior_a.astype(F64), sa + np.abs(prior_a.astype(F64))
    if prior_b is not None:
        db, sb = db + prior_b.astype(F64), sb + np.abs(prior_b.astype(F64))
    return da, sa, db, sb


def ref64_act_bwd(y, dy, act):
    v = act_deriv64(y, act) * dy.astype(F64)
    return v, np.abs(v)


def f32_copy2d(src, dst, rows, cols, accumulate):
    """dst[:rows, :cols] (+)= src[:rows, :cols] on a copy of dst (bits of everything else kept)"""
    out = dst.copy()
    out[:rows, :cols] = (dst[:rows, :cols] + src[:rows, :cols]).astype(F32) if accumulate else src[:rows, :cols]
    return out


# ---------------------------------------------------------------------------------------------------------------
# row marks, `seen` bitmaps and the touched list
#   mark map: field f owns bytes [markbase[f], markbase[f] + V_f), markbase[f] = 32 sum_{g < f} ceil(V_g / 32)
#   bitmap:   bit (r & 31) of word r >> 5 of field f's own array of ceil(V_f / 32) words
#   list:     global row ids rowbase[f] + r, rowbase = prefix sum of V
# ---------------------------------------------------------------------------------------------------------------
def words_of(V):
    return (int(V) + 31) // 32


def mark_layout(vocab):
    """(markbase per field, bytes of the whole map)"""
    base, w = [], 0
    for v in vocab:
        base.append(32 * w)
        w += words_of(v)
    return base, 32 * w


def row_base(vocab):
    rb = [0]
    for v in vocab:
        rb.append(rb[-1] + int(v))
    return rb


def clamp_rows(idx, vocab):
    """mml_gather_fwd's range handling: (clamped [B, F] rows, status bits: 1 = a negative index, 2 = one >= V)"""
    idx = np.asarray(idx, dtype=np.int64)
    V = np.asarray(vocab, dtype=np.int64)[None, :]
    status = (1 if (idx < 0).any() else 0) | (2 if (idx >= V).any() else 0)
    return np.clip(idx, 0, V - 1), status


def ref_mark_map(rows, vocab):
    """byte map after mml_gather_fwd_mark on an all-zero map: 1 at markbase[f] + r for every r in rows[:, f], else 0"""
    base, total = mark_layout(vocab)
    m = np.zeros(total, np.uint8)
    for f in range(len(vocab)):
        m[base[f] + np.unique(rows[:, f])] = 1
    return m


def rows_to_bitmap(rows, V):
    w = np.zeros(words_of(V), np.uint32)
    rows = np.unique(np.asarray(rows, dtype=np.int64))
    assert rows.size == 0 or (rows[0] >= 0 and rows[-1] < V)
    np.bitwise_or.at(w, rows >> 5, (np.uint32(1) << (rows & 31).astype(np.uint32)))
    return w


def bitmap_to_rows(words):
    bits = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")
    return np.flatnonzero(bits).astype(np.int64)


def ref_compact(seen, marked, vocab):
    """seen: uint32 bitmap per field; marked: rows per field, or None (no mark map: the bitmaps hold the marks).
    Returns (sorted global ids of the list, the bitmaps afterwards = old | marks)."""
    rb = row_base(vocab)
    ids, after = [], []
    for f, V in enumerate(vocab):
        w = seen[f].copy() if marked is None else seen[f] | rows_to_bitmap(marked[f], V)
        after.append(w)
        ids.append(bitmap_to_rows(w) + rb[f])
    return np.concatenate(ids), after


def build_compact(vocab, seed, n_old=None, n_new=None):
    """Old `seen` rows and new marks per field such that, where the field is large enough, its words hold only old
    bits, only new marks, both, and neither: rows of word 4 j + 0 are old, of 4 j + 1 new, of 4 j + 2 both kinds; word
    4 j + 3 stays empty.  Tiny fields get what fits (row 0 old and new for V = 1)."""
    rng = np.random.default_rng(seed)
    old, new = [], []
    for f, V in enumerate(vocab):
        V = int(V)
        k_old = min(V, n_old if n_old is not None else max(1, V // 7))
        k_new = min(V, n_new if n_new is not None else max(1, V // 5))
        o, m = rng.choice(V, k_old, replace=False), rng.choice(V, k_new, replace=False)
        wo, wm = (o >> 5) & 3, (m >> 5) & 3
        o, m = o[(wo == 0) | (wo == 2)], m[(wm == 1) | (wm == 2)]
        if V <= 32 * 4:  # a field of a few words: both kinds in word 0 whatever the draw gave
            o, m = np.append(o, 0), np.append(m, [min(V - 1, 5), V - 1])  # (and the last row, marked)
        old.append(np.unique(o))
        new.append(np.unique(m))
    return old, new


def word_census(old, new, V):
    """number of words of a field holding (only old bits, only new marks, both, neither)"""
    wo, wm = rows_to_bitmap(old, V) != 0, rows_to_bitmap(new, V) != 0
    return int((wo & ~wm).sum()), int((~wo & wm).sum()), int((wo & wm).sum()), int((~wo & ~wm).sum())


MARK_VOCABS = (1, 31, 32, 33, 1000)
GATHER_B = (1, 257, 4096)
GATHER_F = (1, 3, MAX_FIELDS)
GATHER_ND = (0, 5)
GATHER_FORMS = (("vec4", 8, 0), ("scalar_E6", 6, 0), ("scalar_ldo", 8, 1))  # (name, E, ldo % 4)


def gather_vocab(F, shift):
    return [MARK_VOCABS[(f + shift) % len(MARK_VOCABS)] for f in range(F)]


def build_gather(B, F, Nd, E, shift, seed):
    """tables, X [B, F + Nd + 2] (field f in column col[f] = F - 1 - f, dense columns behind, two unused columns),
    rows [B, F]; field 1 (field 0 when F = 1 and V = 1 anyway) has every sample on its last row."""
    rng = np.random.default_rng(seed)
    vocab = gather_vocab(F, shift)
    rows = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int64)
    if F > 1:
        rows[:, 1] = vocab[1] - 1
    col = [F - 1 - f for f in range(F)]
    X = rng.standard_normal((B, F + Nd + 2)).astype(F32)
    for f in range(F):
        X[:, col[f]] = rows[:, f].astype(F32) + F32(0.25)  # (truncation toward zero: the fraction is dropped)
    tabs = [rng.standard_normal((v, E)).astype(F32) for v in vocab]
    return dict(vocab=vocab, rows=rows, col=col, X=X, tabs=tabs, dense_col0=F)


def ref_gather(tabs, rows, X, dense_col0, Nd):
    """[B, F E + Nd] float32: the rows of every field side by side, then the dense columns"""
    parts = [t[rows[:, f]] for f, t in enumerate(tabs)]
    return np.concatenate(parts + [X[:, dense_col0:dense_col0 + Nd]], 1)


# ---------------------------------------------------------------------------------------------------------------
# mml_shard_rows: shard[l] = table[l world + first] (zero rows behind the table's end), and the inverse copy
# ---------------------------------------------------------------------------------------------------------------
SHARD_WORLDS = (1, 2, 3, 8)
SHARD_V = (1, 7, 64, 1000)
SHARD_E = (4, 5, 16)


def ref_shard(table, world, first, rows_local):
    src = table[first::world]
    assert len(src) <= rows_local
    out = np.zeros((rows_local, table.shape[1]), F32)
    out[:len(src)] = src
    return out


def ref_unshard(table, shard, world, first):
    """a copy of `table` whose rows first, first + world, ... < V hold the shard's rows"""
    out = table.copy()
    rows = np.arange(first, table.shape[0], world)
    out[rows] = shard[:len(rows)]
    return out
