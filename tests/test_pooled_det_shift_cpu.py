"""mml_scatter_pool_det_shift (include/mmlrec.h, next to K2p): the fixed-point shift of the deterministic pooled scatter, a
pure host rule -- called here through the library, no device needed.  A row of table tb may receive B * L_tb addends,
L_tb = the single-valued fields on tb + the sum of maxlen over the pooled fields on tb; the rule keeps
24 significand bits + shift + ceil(log2(B * max_tb L_tb)) below 63, never gives more than 28, equals
mml_scatter_det_shift(B) for a single-valued schema with one field per table, and is negative where less than 4 bits
would be left -- there the scatter refuses the batch before it launches anything."""
import ctypes

import pytest


def _desc(E=8, vocab=(100,), singles=(), pooled=()):
    from mmlrec_amd import _lib
    d = _lib.PoolDesc()
    d.n_tables, d.E, d.n_single, d.n_pooled = len(vocab), E, len(singles), len(pooled)
    for i, v in enumerate(vocab):
        d.vocab[i] = v
        d.table[i] = 1 << 20  # (an aligned address that is never dereferenced)
    for i, (c, t) in enumerate(singles):
        d.s_col[i], d.s_table[i] = c, t
    for i, (c0, T, comb, tb, lc) in enumerate(pooled):
        d.p_col0[i], d.p_maxlen[i], d.p_combiner[i], d.p_table[i], d.p_len_col[i] = c0, T, comb, tb, lc
    return d


def _clog2(n):
    return (n - 1).bit_length()  # exact ceil(log2 n) for n >= 1


# (name, vocab, singles, pooled, Lmax)
SCHEMAS = [
    ("one single-valued field", (100,), ((0, 0),), (), 1),
    ("five single-valued fields, a table each", (10, 20, 30, 40, 50), tuple((f, f) for f in range(5)), (), 1),
    ("one pooled field of maxlen 1", (100,), (), ((0, 1, 0, 0, -1),), 1),
    ("one pooled field of maxlen 5", (100,), (), ((0, 5, 1, 0, -1),), 5),
    ("maxlen 256", (100,), (), ((0, 256, 2, 0, -1),), 256),
    ("two single-valued fields on ONE table", (100,), ((0, 0), (1, 0)), (), 2),
    ("an id column and its history share a table", (50, 5000), ((0, 0), (1, 1)), ((2, 20, 1, 1, 22),), 21),
    ("two histories and an id on one table, a longer field elsewhere", (50, 5000, 70), ((0, 0), (1, 1)),
     ((2, 20, 1, 1, -1), (22, 64, 0, 1, -1), (86, 70, 2, 2, -1)), 85),
    ("the widest descriptor: 16 pooled fields of maxlen 256 and 16 single-valued ones on one table", (1000,),
     tuple((f, 0) for f in range(16)), tuple((16 + 256 * p, 256, p % 3, 0, -1) for p in range(16)), 16 + 16 * 256),
]
BATCHES = [0, 1, 2, 3, 64, 1000, 1024, 1025, 65536, 1 << 20, (1 << 24) + 1, 1 << 30, 1 << 34, (1 << 34) + 1, 1 << 40]


@pytest.mark.parametrize("name,vocab,singles,pooled,lmax", SCHEMAS, ids=[s[0] for s in SCHEMAS])
def test_shift_keeps_the_headroom(name, vocab, singles, pooled, lmax):
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib, ops
    lib = _lib.load()
    d = _desc(vocab=vocab, singles=singles, pooled=pooled)
    seen_negative = False
    for B in BATCHES:
        lg = _clog2(max(B, 1) * lmax)
        shift = lib.mml_scatter_pool_det_shift(ctypes.byref(d), B)
        assert shift == ops.scatter_pool_det_shift(d, B)
        if 24 + 4 + lg >= 63:  # beyond the limit: no clamp below 4, a refusal
            assert shift < 0, (B, shift)
            seen_negative = True
            continue
        assert shift == min(28, 62 - 24 - lg), (B, shift)
        assert 4 <= shift <= 28
        assert 24 + shift + lg < 63
    assert seen_negative  # every schema reaches the limit within BATCHES


def test_single_valued_unshared_schema_gives_the_single_valued_rule():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib
    lib = _lib.load()
    d = _desc(vocab=(10, 20, 30), singles=((0, 0), (1, 1), (2, 2)))
    for B in list(range(0, 70)) + [b + k for b in (1 << 10, 1 << 20, 1 << 33, 1 << 34) for k in (-1, 0)] + [(1 << 10) + 1]:
        assert lib.mml_scatter_pool_det_shift(ctypes.byref(d), B) == lib.mml_scatter_det_shift(B), B
    # a pooled field of maxlen 1 is one lookup per sample as well
    p = _desc(vocab=(10, 20), singles=((0, 0),), pooled=((1, 1, 0, 1, -1),))
    for B in (1, 1000, 65536, 1 << 30):
        assert lib.mml_scatter_pool_det_shift(ctypes.byref(p), B) == lib.mml_scatter_det_shift(B), B


def test_shared_tables_fields_count_together_and_the_largest_table_decides():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib, ops
    lib = _lib.load()
    B = 1 << 20
    # (B = 2^20: shift = 38 - 20 - ceil(log2 L) is below the cap of 28 for every L >= 1, so L shows in the result)
    own = _desc(vocab=(100, 100), singles=((0, 0),), pooled=((1, 4, 0, 1, -1),))       # L = (1, 4)
    shared = _desc(vocab=(100,), singles=((0, 0),), pooled=((1, 4, 0, 0, -1),))        # L = 5: one more bit
    assert lib.mml_scatter_pool_det_shift(ctypes.byref(own), B) == 38 - 20 - 2
    assert lib.mml_scatter_pool_det_shift(ctypes.byref(shared), B) == 38 - 20 - 3
    two = _desc(vocab=(100,), singles=((0, 0), (1, 0)))                                 # two id columns on one table
    assert lib.mml_scatter_pool_det_shift(ctypes.byref(two), B) == 38 - 20 - 1
    # the same rule from field lists
    assert ops.scatter_pool_det_shift(([100], 8, [(0, 0)], [ops.PooledField(1, 4, "sum", 0)]), B) == 38 - 20 - 3


def test_refusals_need_no_device():
    """A malformed descriptor has no shift; the entry point checks its required buffers, its flags and the headroom
    before any launch (the addresses below are never dereferenced)."""
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib
    lib = _lib.load()
    assert "mml_scatter_pool_bwd_det" in _lib.EXPORTS and "mml_scatter_pool_det_shift" in _lib.EXPORTS
    assert lib.mml_scatter_pool_det_shift(None, 64) < 0
    assert lib.mml_scatter_pool_det_shift(ctypes.byref(_desc(E=12, singles=((0, 0),))), 64) < 0
    assert lib.mml_scatter_pool_det_shift(ctypes.byref(_desc(singles=((0, 0),))), -1) < 0
    d = _desc(pooled=((0, 5, 1, 0, -1),))
    p = 1 << 20
    acc = (ctypes.c_void_p * 1)(p)
    call = lambda d=d, B=4, acc=acc, slot=p, marks=p, flags=0: lib.mml_scatter_pool_bwd_det(  # noqa: E731
        ctypes.byref(d), p, 64, B, p, 64, None, 0, acc, slot, marks, flags, None, None)
    assert call(d=_desc(E=12)) == _lib.ERR_ARG
    assert call(acc=None) == _lib.ERR_ARG and b"acc64" in lib.mml_last_error()
    assert call(acc=(ctypes.c_void_p * 1)(None)) == _lib.ERR_ARG and b"acc64[0]" in lib.mml_last_error()
    assert call(slot=None) == _lib.ERR_ARG and call(marks=None) == _lib.ERR_ARG
    assert call(flags=8) == _lib.ERR_ARG and b"flag" in lib.mml_last_error()
    assert call(flags=_lib.SCATTER_DET_DEFER_TOTALS | _lib.SCATTER_DET_CLEAR_MARKS) == _lib.ERR_ARG
    assert call(B=1 << 33) == _lib.ERR_ARG and b"headroom" in lib.mml_last_error()  # 2^33 samples x 5 positions
    assert call(B=0) == 0  # an empty batch launches nothing
