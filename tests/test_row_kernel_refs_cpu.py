"""Host-side proof of tests/row_kernel_refs.py, without a GPU:
  * every numpy reference agrees with a deliberately naive per-element Python loop at tiny sizes;
  * the mark-map, bitmap and list layouts are checked at V = 1, 31, 32, 33;
  * the unmutated float32 restatement of sumprod stays inside the derived tolerance on every input the GPU file uses,
    and each named mutation (the last term's y ignored, the prior dropped when accumulating, sigmoid' used for sigmoid2)
    is rejected on every item where it can apply; the bit-exact cases are bit-exact on the host as well;
  * the compaction inputs really hold words with only old bits, only new marks, both and neither."""
import math

import numpy as np
import pytest

import row_kernel_refs as R
from row_kernel_refs import F32, F64, assert_close_terms, bits_equal


def rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def f64(v):
    return float(F64(F32(v)))


# ---------------------------------------------------------------------------------------------------------------
# sumprod
# ---------------------------------------------------------------------------------------------------------------
def _naive_deriv(o, act):
    o = f64(o)
    return {R.ACT_NONE: 1.0, R.ACT_RELU: 1.0 if o > 0 else 0.0, R.ACT_SIGMOID: o * (1 - o),
            R.ACT_SIGMOID2: o * (1 - o / 2)}[act]


def _naive_sumprod(it):
    out, sa = [], []
    for i in range(it["n"]):
        s = f64(it["prior"][i]) if it["accumulate"] else 0.0
        a = abs(s)
        for x, y in zip(it["xs"], it["ys"]):
            t = f64(x[i]) * (f64(y[i]) if y is not None else 1.0)
            s, a = s + t, a + abs(t)
        if it["act"]:
            d = _naive_deriv(it["deriv_of"][i], it["act"])
            s, a = s * d, a * abs(d)
        out.append(s)
        sa.append(a)
    return np.array(out, F64), np.array(sa, F64)


TINY_ITEMS = ([R.build_sumprod(6, nt, pat, acc, R.ACT_NONE, seed=nt * 10 + acc)
               for nt in (0, 1, 3, 8) for pat in R.Y_PATTERNS for acc in (0, 1)] +
              [R.build_sumprod(7, nt, "last_null", 0, act, seed=act) for act in R.ACTS for nt in (0, 2)])


def test_sumprod_reference_against_a_per_element_loop():
    for it in TINY_ITEMS:
        ref, sa = R.ref64_sumprod_item(it)
        nref, nsa = _naive_sumprod(it)
        assert ref.shape == (it["n"],)
        assert_close_terms(ref, nref, np.maximum(nsa, 1e-300), 1e-15, "sumprod ref vs loop")
        assert_close_terms(sa, nsa, np.maximum(nsa, 1e-300), 1e-15, "sumprod sumabs vs loop")


def test_y_patterns_and_specials():
    assert R.y_pattern("none", 3) == [False] * 3 and R.y_pattern("all", 3) == [True] * 3
    assert R.y_pattern("last_null", 3) == [True, True, False] and R.y_pattern("first_null", 3) == [False, True, True]
    assert R.y_pattern("last_null", 1) == [False] and R.y_pattern("all", 0) == []
    for act in R.ACTS:
        o = R.act_outputs(act, 50, np.random.default_rng(act))
        assert o[0] == 0 and not np.signbit(o[0]) and o[1] == 1 and o[2] == 2 and o[3] == 0 and np.signbit(o[3])
        d = R.act_deriv64(o, act)
        assert d[0] == 0 and d[3] == 0  # relu'(-0) = 0 too
        assert d[2] == (1.0 if act == R.ACT_RELU else -2.0 if act == R.ACT_SIGMOID else 0.0)  # sigmoid2 saturated
        for i in range(50):
            assert math.isclose(d[i], _naive_deriv(o[i], act), rel_tol=1e-15, abs_tol=0)
        assert bits_equal(R.act_deriv32(o, act)[:4], R.act_deriv64(o, act)[:4].astype(F32))


def _all_gpu_items():
    items = []
    for n in (1029, 1028):
        for acc in (0, 1):
            items += R.sumprod_term_items(n, acc)
        items += R.sumprod_act_items(n)
    for k in (1, 16, 17, 33):
        items += R.sumprod_mixed_items(k)
    items += [R.sumprod_path_base(m) for m in ("act", "accumulate", "plain")] + R.sumprod_amax_items()[0]
    items += [R.build_sumprod(1024, 1, "none", acc, R.ACT_NONE, seed=43 + acc) for acc in (0, 1)]
    items += R.sumprod_length_items(0) + R.sumprod_length_items(1)
    items += [R.build_sumprod(0, i % 3, "all", i % 2, R.ACT_NONE, seed=i) for i in range(16)]
    items.append(R.build_sumprod(517, 3, "all", 1, R.ACT_NONE, 9))
    return items


def test_sumprod_model_passes_and_every_mutation_is_rejected():
    applied = {m: 0 for m in R.SUMPROD_MUTATIONS}
    exact = 0
    for it in _all_gpu_items():
        ref, sa = R.ref64_sumprod_item(it)
        tol = R.sumprod_tol(it["n_terms"])
        assert_close_terms(R.model32_sumprod(it), ref, sa, tol, "model32_sumprod: unmutated")
        ex = R.sumprod_exact32(it)
        if ex is not None:
            exact += 1
            assert bits_equal(R.model32_sumprod(it), ex)
        for m in R.SUMPROD_MUTATIONS:
            got = R.model32_sumprod(it, m)
            if R.sumprod_mutation_applies(it, m):
                applied[m] += 1
                assert rejected(lambda: assert_close_terms(got, ref, sa, tol, "mutated")), (m, it["n"], it["n_terms"])
            else:  # (nothing for the mutation to change: still inside)
                assert_close_terms(got, ref, sa, tol, "model32_sumprod: mutation without effect")
    assert all(v >= 8 for v in applied.values()), applied
    assert exact >= 8


def test_sumprod_case_lists_cover_what_the_device_test_claims():
    for k in (1, 16, 17, 33):
        items = R.sumprod_mixed_items(k)
        assert len(items) == k
        assert len({(it["n"], it["n_terms"], it["ypat"], it["accumulate"], it["act"]) for it in items}) == k
    items = R.sumprod_mixed_items(33)
    assert {it["act"] for it in items} == {0, 1, 2, 3} and {it["accumulate"] for it in items} == {0, 1}
    assert {it["n_terms"] for it in items} == set(range(9))
    assert {it["n"] % 4 == 0 for it in items} == {True, False}
    terms = R.sumprod_term_items(1028, 0)
    assert len(terms) == 20 and {(it["n_terms"], it["ypat"]) for it in terms} == {
        (nt, p) for nt in R.SUMPROD_NTERMS for p in R.Y_PATTERNS}
    assert R.SUMPROD_SCALAR_TWO_TRIPS % 4 != 0 and R.SUMPROD_SCALAR_TWO_TRIPS > 128 * 256
    assert R.SUMPROD_VEC_TWO_TRIPS % 4 == 0 and R.SUMPROD_VEC_TWO_TRIPS // 4 > 128 * 256
    assert max(2048 // R.SUMPROD_BATCH, 64) == 128


# ---------------------------------------------------------------------------------------------------------------
# elementwise neighbours
# ---------------------------------------------------------------------------------------------------------------
def test_elementwise_references_against_loops():
    n = 9
    w = R.build_ew(n, 3)
    ins = [w["a"], w["b"], w["d"]]
    s = R.f32_add_n(ins)
    for i in range(n):
        acc = F32(0)
        for x in ins:
            acc = F32(acc + x[i])
        assert acc == s[i]
    for act_a, act_b in ((0, 0), (1, 3), (2, 1), (3, 2)):
        for pa, pb in ((None, None), (w["pa"], w["pb"])):
            da, sa, db, sb = R.ref64_mul_bwd(w["d"], w["a"], w["b"], pa, pb, act_a, act_b)
            for i in range(n):
                va = f64(w["d"][i]) * f64(w["b"][i]) * _naive_deriv(w["a"][i], act_a)
                vb = f64(w["d"][i]) * f64(w["a"][i]) * _naive_deriv(w["b"][i], act_b)
                ea, eb = (f64(pa[i]), f64(pb[i])) if pa is not None else (0.0, 0.0)
                assert math.isclose(da[i], va + ea, rel_tol=1e-14) and math.isclose(db[i], vb + eb, rel_tol=1e-14)
                assert math.isclose(sa[i], abs(va) + abs(ea), rel_tol=1e-14)
                assert math.isclose(sb[i], abs(vb) + abs(eb), rel_tol=1e-14)
    for act in R.ACTS:
        y = R.act_outputs(act, n, np.random.default_rng(act))
        v, sa = R.ref64_act_bwd(y, w["d"], act)
        for i in range(n):
            assert math.isclose(v[i], _naive_deriv(y[i], act) * f64(w["d"][i]), rel_tol=1e-15, abs_tol=0)
            assert sa[i] == abs(v[i])
    src = np.arange(12, dtype=F32).reshape(3, 4)
    dst = np.full((4, 6), np.nan, F32)
    dst[:3, :2] = 1
    out = R.f32_copy2d(src, dst, 3, 2, 1)
    assert np.array_equal(out[:3, :2], src[:3, :2] + 1) and np.isnan(out[:, 2:]).all() and np.isnan(out[3]).all()
    out = R.f32_copy2d(src, dst, 3, 2, 0)
    assert np.array_equal(out[:3, :2], src[:3, :2]) and np.isnan(out[:, 2:]).all()


# ---------------------------------------------------------------------------------------------------------------
# marks, bitmaps, list
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 31, 32, 33])
def test_layout_helpers(V):
    assert R.words_of(V) == (1 if V <= 32 else 2)
    vocab = [V, 5, V]
    base, total = R.mark_layout(vocab)
    assert base == [0, 32 * R.words_of(V), 32 * R.words_of(V) + 32] and total == 64 * R.words_of(V) + 32
    assert all(b % 32 == 0 for b in base)
    assert R.row_base(vocab) == [0, V, V + 5, 2 * V + 5]
    # bitmap: bit r & 31 of word r >> 5, both ways, for every row alone and for all together
    for r in range(V):
        w = R.rows_to_bitmap([r], V)
        assert len(w) == R.words_of(V) and int(w[r >> 5]) == 1 << (r & 31) and int(w.sum()) == 1 << (r & 31)
        assert R.bitmap_to_rows(w).tolist() == [r]
    w = R.rows_to_bitmap(np.arange(V), V)
    assert R.bitmap_to_rows(w).tolist() == list(range(V))
    assert int(w[-1]) == (1 << ((V - 1) % 32 + 1)) - 1  # no bit behind V
    assert R.rows_to_bitmap([], V).sum() == 0 and R.bitmap_to_rows(np.zeros(2, np.uint32)).size == 0
    # mark map: naive loop
    rng = np.random.default_rng(V)
    rows = np.stack([rng.integers(0, v, 6) for v in vocab], 1)
    m = R.ref_mark_map(rows, vocab)
    naive = [0] * total
    for b in range(6):
        for f in range(3):
            naive[32 * sum((vocab[g] + 31) // 32 for g in range(f)) + int(rows[b, f])] = 1
    assert m.tolist() == naive
    for f, v in enumerate(vocab):  # tail bytes between V_f and the next field's base stay 0
        assert not m[base[f] + v:base[f] + 32 * R.words_of(v)].any()


def test_clamp_rows():
    idx = np.array([[0, 4], [-3, 2], [1, 9]])
    rows, st = R.clamp_rows(idx, [2, 5])
    assert rows.tolist() == [[0, 4], [0, 2], [1, 4]] and st == 3
    assert R.clamp_rows([[0, 0]], [2, 5])[1] == 0 and R.clamp_rows([[-1, 0]], [2, 5])[1] == 1
    assert R.clamp_rows([[2, 0]], [2, 5])[1] == 2


@pytest.mark.parametrize("vocab", [[1], [31, 32, 33], [1000, 1, 33], [32 * 1024 + 1]])
def test_compact_reference_against_a_loop(vocab):
    old, new = R.build_compact(vocab, seed=len(vocab))
    seen = [R.rows_to_bitmap(o, v) for o, v in zip(old, vocab)]
    for marked in (new, None):
        ids, after = R.ref_compact(seen, marked, vocab)
        want, base = [], 0
        for f, v in enumerate(vocab):
            rows = set(old[f].tolist()) | (set(new[f].tolist()) if marked is not None else set())
            want += [base + r for r in sorted(rows)]
            for r in range(v):
                assert bool((int(after[f][r >> 5]) >> (r & 31)) & 1) == (r in rows)
            base += v
        assert ids.tolist() == want and len(set(want)) == len(want)
    assert all(np.array_equal(a, s) for a, s in zip(R.ref_compact(seen, None, vocab)[1], seen))


def test_compact_inputs_hold_the_four_kinds_of_word():
    for V in (1000, 32 * 1024, 32 * 1024 + 1):
        (old,), (new,) = R.build_compact([V], seed=V)
        only_old, only_new, both, neither = R.word_census(old, new, V)
        assert min(only_old, only_new, both, neither) >= 1, (V, only_old, only_new, both, neither)
    for V in (1, 31, 32, 33):  # one or two words: old bits and new marks share word 0
        (old,), (new,) = R.build_compact([V], seed=V)
        assert R.word_census(old, new, V)[2] >= 1
    assert R.word_census([0], [40], 100) == (1, 1, 0, 2) and R.word_census([0, 40], [40], 100) == (1, 0, 1, 2)


def test_gather_builder_and_reference():
    for B, F, Nd, E in ((1, 1, 0, 8), (5, 3, 5, 6), (4, R.MAX_FIELDS, 5, 8)):
        for shift in range(3):
            g = R.build_gather(B, F, Nd, E, shift, seed=B + F)
            assert sorted(g["col"]) == list(range(F)) and g["dense_col0"] == F
            assert all(0 <= g["rows"][:, f].min() and g["rows"][:, f].max() < v for f, v in enumerate(g["vocab"]))
            assert np.array_equal(g["X"][:, g["col"]].astype(np.int64), g["rows"])  # truncation toward zero
            if F > 1:
                assert (g["rows"][:, 1] == g["vocab"][1] - 1).all()
            ref = R.ref_gather(g["tabs"], g["rows"], g["X"], F, Nd)
            assert ref.shape == (B, F * E + Nd)
            for b in range(B):
                for f in range(F):
                    assert bits_equal(ref[b, f * E:(f + 1) * E], g["tabs"][f][g["rows"][b, f]])
                assert bits_equal(ref[b, F * E:], g["X"][b, F:F + Nd])
    assert set(R.gather_vocab(R.MAX_FIELDS, 0)) == set(R.MARK_VOCABS)
    assert [R.gather_vocab(1, s)[0] for s in range(3)] == [1, 31, 32]


# ---------------------------------------------------------------------------------------------------------------
# shards
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", R.SHARD_WORLDS)
@pytest.mark.parametrize("V", [1, 7, 64])
def test_shard_reference_against_a_loop(world, V):
    E = 3
    table = np.random.default_rng(V).standard_normal((V, E)).astype(F32)
    rebuilt = np.full((V, E), np.nan, F32)
    for first in range(world):
        for rows_local in ((V + world - 1) // world, (V + world - 1) // world + 2):
            sh = R.ref_shard(table, world, first, rows_local)
            assert sh.shape == (rows_local, E)
            for l in range(rows_local):
                r = l * world + first
                assert bits_equal(sh[l], table[r] if r < V else np.zeros(E, F32))
        back = R.ref_unshard(rebuilt, sh, world, first)
        for r in range(V):  # (the ranks before this one have written theirs already)
            assert bits_equal(back[r], table[r]) if r % world <= first else np.isnan(back[r]).all()
        rebuilt = back
    assert bits_equal(rebuilt, table)
