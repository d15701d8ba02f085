"""The optimizer's planning rules, which need no GPU: dense_table_launches (the mml_opt_step_dense calls of the dense table
update), resolve_table_update (the table-update mode) and OptKnobs.from_env.  Every expectation is the rule list of the
functions' docstrings written out; every launch planned here is also held against the C side's size rule
(csrc/opt_plan.hpp, which mml_opt_step_dense launches by), asked of the compiled rule itself in c_side_streams below."""
import pytest

E8 = 8
AE30_ROWS = [10_000_000] + [1_000_000] * 2 + [100_000] * 4 + [10_000] * 8 + [1_000] * 8 + [100] * 6 + [2]
PER = {"sgd": 12, "adam": 28, "adagrad": 20, "rmsprop": 20}
BIG, SMALL = (0, 1, 2), tuple(range(3, 30))
CAP = 1 << 20


@pytest.fixture()
def mod():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, optimizer as O
    return O, L


def c_side_streams(total, n, all_marked):
    """Whether the C rule streams `total` parameters in `n` tensors (csrc/opt_plan.hpp through the stand-alone driver of
    test_opt_plan_cpu.py); a marked group the flat kernel would get is refused there: it does not stream."""
    from test_opt_plan_cpu import run_plans
    sizes = [total - (n - 1)] + [1] * (n - 1)
    marks = (1 << 20) if all_marked else 0
    return isinstance(run_plans([([(s, E8, marks, 0, 0, 0) for s in sizes], CAP, 0, {})])[0], dict)


def plan(O, rows, marks=True, kind="adam", split=False, cap=CAP, deferred=False, E=E8, **knobs):
    """dense_table_launches over tables of `rows` x E; every launch checked against the C rule: one that does not stream
    carries no marks (the flat kernel refuses them), and the label says opt_flat_kernel exactly then."""
    numels = [r * E for r in rows]
    marks = [marks] * len(rows) if isinstance(marks, bool) else marks
    out = O.dense_table_launches(kind, numels, rows, marks, split, cap, deferred, O.OptKnobs(**knobs))
    for ln in out:
        streams = c_side_streams(sum(numels[i] for i in ln.tables), len(ln.tables), ln.marked)
        assert streams or not ln.marked
        assert (ln.kernel == "opt_flat_kernel") == (not streams)
        assert ln.kernel == "opt_flat_kernel" or ln.kernel.startswith("opt_dense_kernel<true, %d, " % ln.form)
    assert sorted(i for ln in out for i in ln.tables) == list(range(len(rows)))  # every table in exactly one launch
    return [tuple(ln) for ln in out]


def nbytes(rows, grp, marked, kind="adam", split=False, E=E8):
    n = (PER[kind] - (4 if split else 0)) * sum(rows[i] * E for i in grp)
    return float(n + (sum(rows[i] - 4 * rows[i] * E for i in grp) if marked else 0))


# ---- dense_table_launches -------------------------------------------------------------------------------------------
def test_ae30_marked(mod):
    O, _ = mod
    assert [AE30_ROWS[i] * E8 for i in BIG] == [80_000_000, 8_000_000, 8_000_000]
    assert plan(O, AE30_ROWS) == [
        (BIG, True, 3, nbytes(AE30_ROWS, BIG, True), "opt_dense_kernel<true, 3, 2>"),
        (SMALL, False, 0, nbytes(AE30_ROWS, SMALL, False), "opt_flat_kernel")]
    assert plan(O, AE30_ROWS, opt_u=4)[0][4] == "opt_dense_kernel<true, 3, 4>"
    # one unmarked table: the big launch reads every gradient
    marks = [i != 1 for i in range(30)]
    assert plan(O, AE30_ROWS, marks=marks) == [
        (BIG, False, 0, nbytes(AE30_ROWS, BIG, False), "opt_dense_kernel<true, 0, 1>"),
        (SMALL, False, 0, nbytes(AE30_ROWS, SMALL, False), "opt_flat_kernel")]


def test_ae30_one_launch(mod):
    O, _ = mod
    every = SMALL + BIG  # small tables first
    assert plan(O, AE30_ROWS, one_launch=True) == [
        (every, True, 3, nbytes(AE30_ROWS, every, True), "opt_dense_kernel<true, 3, 2>")]
    # needs cap > 0, every table marked, no split, at most MAX_OPT_TENSORS tables
    assert len(plan(O, AE30_ROWS, one_launch=True, cap=0)) == 2
    assert len(plan(O, AE30_ROWS, one_launch=True, marks=[i != 29 for i in range(30)])) == 2
    assert len(plan(O, AE30_ROWS, one_launch=True, marks=False, split=True)) == 2
    assert len(plan(O, AE30_ROWS + [100] * 3, one_launch=True)) == 2
    # and both groups: all tables small, or all big -> the one launch there is anyway
    assert len(plan(O, AE30_ROWS[3:], one_launch=True)) == 1
    assert plan(O, AE30_ROWS[:3], one_launch=True)[0][0] == (0, 1, 2)


def test_ae30_deferred_totals(mod):
    O, _ = mod
    every = SMALL + BIG
    for cap in (CAP, 0):  # (any grid)
        assert plan(O, AE30_ROWS, deferred=True, cap=cap) == [
            (every, True, 4, nbytes(AE30_ROWS, every, True), "opt_dense_kernel<true, 4, 2>")]
    assert plan(O, AE30_ROWS, deferred=True, opt_u=4)[0][4] == "opt_dense_kernel<true, 4, 4>"
    assert plan(O, AE30_ROWS, deferred=True, opt_u=8)[0][4] == "opt_dense_kernel<true, 4, 2>"


def test_ae30_no_cap(mod):
    O, _ = mod
    assert plan(O, AE30_ROWS, cap=0) == [
        (BIG, True, 0, nbytes(AE30_ROWS, BIG, True), "opt_dense_kernel<true, 0, 1>"),
        (SMALL, False, 0, nbytes(AE30_ROWS, SMALL, False), "opt_flat_kernel")]


def test_ae30_fifth_scale_has_no_big_group(mod):
    O, _ = mod
    rows = [max(2, int(v * 0.2)) for v in AE30_ROWS]
    numels = [r * E8 for r in rows]
    assert numels[:3] == [16_000_000, 1_600_000, 1_600_000]
    assert [n >= (1 << 22) for n in numels] == [True] + [False] * 29  # only the first is huge ...
    assert numels[0] < (1 << 24) < sum(numels)                        # ... and alone it is no streaming launch
    every = tuple(range(30))
    assert plan(O, rows) == [(every, False, 0, nbytes(rows, every, False), "opt_flat_kernel")]


def test_more_than_four_huge_tables(mod):
    O, _ = mod
    rows = [(1 << 22) // E8] * 5
    assert 5 * (1 << 22) >= (1 << 24)
    every = tuple(range(5))
    assert plan(O, rows) == [(every, False, 0, nbytes(rows, every, False), "opt_flat_kernel")]
    four = tuple(range(4))  # (four of them: exactly 2^24, one marked streaming launch)
    assert plan(O, rows[:4]) == [(four, True, 3, nbytes(rows, four, True), "opt_dense_kernel<true, 3, 2>")]
    assert plan(O, [rows[0] - 1] + rows[:3])[0][4] == "opt_flat_kernel"


def test_split_update(mod):
    O, _ = mod
    for cap, form, label in ((512, 2, "opt_dense_kernel<true, 2, 4>"), (0, 0, "opt_dense_kernel<true, 0, 1>")):
        assert plan(O, AE30_ROWS, marks=False, split=True, cap=cap) == [
            (BIG, False, form, nbytes(AE30_ROWS, BIG, False, split=True), label),
            (SMALL, False, form, nbytes(AE30_ROWS, SMALL, False, split=True), "opt_flat_kernel")]
    assert nbytes(AE30_ROWS, BIG, False, split=True) == 24.0 * 96_000_000


def test_variant_two_chunks(mod):
    O, _ = mod
    assert plan(O, AE30_ROWS, marks=False, variant=2) == [
        (BIG, False, 1, nbytes(AE30_ROWS, BIG, False), "opt_dense_kernel<true, 1, 1>"),
        (SMALL, False, 1, nbytes(AE30_ROWS, SMALL, False), "opt_flat_kernel")]
    # marked or split launches keep their own form
    assert [ln[2] for ln in plan(O, AE30_ROWS, variant=2)] == [3, 1]
    assert [ln[2] for ln in plan(O, AE30_ROWS, marks=False, split=True, cap=512, variant=2)] == [2, 2]
    assert [ln[2] for ln in plan(O, AE30_ROWS, marks=False, split=True, cap=0, variant=2)] == [0, 0]
    assert [ln[2] for ln in plan(O, AE30_ROWS, marks=False, variant=1)] == [0, 0]


def test_deferred_totals_refused(mod):
    O, L = mod
    numels = [r * E8 for r in AE30_ROWS]
    k = O.OptKnobs()
    ok = dict(kind="adam", numels=numels, rows=AE30_ROWS, marks=[True] * 30, split_dense=False, cap=CAP,
              det_deferred=True, knobs=k)
    assert len(O.dense_table_launches(**ok)) == 1
    for bad in (dict(split_dense=True, marks=[False] * 30), dict(marks=[True] * 29 + [False]), dict(det_exact=False)):
        with pytest.raises(L.MMLError, match="deferred its totals to a marked dense update of exactly its tables"):
            O.dense_table_launches(**dict(ok, **bad))
    # the one launch must stream: below 2^24 parameters the flat kernel would get the totals
    rows = [max(2, int(v * 0.05)) for v in AE30_ROWS]
    assert sum(rows) * E8 < (1 << 24)
    with pytest.raises(L.MMLError):
        O.dense_table_launches(**dict(ok, numels=[r * E8 for r in rows], rows=rows))


@pytest.mark.parametrize("kind", ["sgd", "adam", "adagrad", "rmsprop"])
def test_bytes_per_kind(mod, kind):
    O, _ = mod
    per = {"sgd": 12, "adam": 28, "adagrad": 20, "rmsprop": 20}[kind]
    big, small = plan(O, AE30_ROWS, kind=kind)
    assert big[3] == per * 96_000_000 + (12_000_000 - 4 * 96_000_000)
    assert small[3] == per * (sum(AE30_ROWS) - 12_000_000) * E8
    big, small = plan(O, AE30_ROWS, kind=kind, marks=False, split=True, cap=0)
    assert (big[3], small[3]) == ((per - 4) * 96_000_000, (per - 4) * (sum(AE30_ROWS) - 12_000_000) * E8)


def test_label_and_deferral_use_the_launch_rule(mod):
    O, L = mod
    assert (L.OPT_STREAM_MIN_PARAMS, L.OPT_HUGE_MIN_PARAMS, L.OPT_STREAM_MAX_TENSORS) == (1 << 24, 1 << 22, 4)
    for total in ((1 << 24) - 1, 1 << 24):
        for n in (1, 4, 5, 30):
            for marked in (False, True):
                assert L.opt_dense_streams(total, n, marked) == c_side_streams(total, n, marked)
                assert (O.opt_dense_symbol(total, n, 3 if marked else 0) == "opt_flat_kernel") == \
                    (not c_side_streams(total, n, marked))
    # what the deterministic scatter asks before it defers is what the optimizer accepts
    assert L.opt_takes_det_totals([1 << 23] * 2, True)
    assert L.opt_takes_det_totals([1 << 19] * L.MAX_OPT_TENSORS, True)
    assert not L.opt_takes_det_totals([1 << 23] * 2, False)
    assert not L.opt_takes_det_totals([1 << 23] * 2, True, split=True)
    assert not L.opt_takes_det_totals([(1 << 23) - 1, 1 << 23], True)
    assert not L.opt_takes_det_totals([1 << 19] * (L.MAX_OPT_TENSORS + 1), True)


# ---- resolve_table_update -------------------------------------------------------------------------------------------
def resolve(O, kind, requested="auto", widths=(8,), one=True, params=1 << 23, reg=None, **knobs):
    return O.resolve_table_update(kind, requested, set(widths), one, params, reg, O.OptKnobs(**knobs))


@pytest.mark.parametrize("kind", ["sgd", "adagrad"])
def test_resolve_sgd_adagrad(mod, kind):
    O, _ = mod
    assert resolve(O, kind) == "sparse_rows"
    assert resolve(O, kind, "lazy_exact") == "sparse_rows"  # (nothing to replay)
    assert resolve(O, kind, "sparse_rows") == "sparse_rows"
    assert resolve(O, kind, "dense_exact") == "dense_exact"
    assert resolve(O, kind, widths=(32,), one=False, params=10) == "sparse_rows"


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_resolve_adam_rmsprop_auto(mod, kind):
    O, _ = mod
    for w in (4, 8, 16):
        assert resolve(O, kind, widths=(w,)) == "lazy_exact"
    assert resolve(O, kind, widths=(4, 8)) == "dense_exact"   # one width only
    assert resolve(O, kind, widths=(32,)) == "dense_exact"
    assert resolve(O, kind, widths=(12,)) == "dense_exact"
    assert resolve(O, kind, widths=()) == "dense_exact"       # no tables
    assert resolve(O, kind, one=False) == "dense_exact"       # shared tables
    assert resolve(O, kind, params=(1 << 22) + 1) == "lazy_exact"
    assert resolve(O, kind, params=1 << 22) == "dense_exact"  # "more than" lazy_min_params
    assert resolve(O, kind, params=2, lazy_min_params=1) == "lazy_exact"
    assert resolve(O, kind, auto_table_update="dense_exact") == "dense_exact"
    for mode in ("dense_exact", "sparse_rows", "lazy_exact"):  # a request is taken as it is
        assert resolve(O, kind, mode, widths=(32,), one=False, params=1, auto_table_update="dense_exact") == mode


def test_resolve_table_regulariser(mod):
    O, _ = mod
    reg = (0.0, 1e-5)
    for kind in ("sgd", "adam", "adagrad", "rmsprop"):
        assert resolve(O, kind, reg=reg) == "dense_exact"
    assert resolve(O, "adam", "lazy_exact", reg=reg) == "lazy_exact"  # under 'auto' only
    assert resolve(O, "adagrad", "sparse_rows", reg=reg) == "sparse_rows"


def test_resolve_unknown_name(mod):
    O, _ = mod
    for kind in ("sgd", "adam"):
        with pytest.raises(ValueError, match="table_update must be auto, dense_exact, sparse_rows or lazy_exact"):
            resolve(O, kind, "dense")


# ---- OptKnobs -------------------------------------------------------------------------------------------------------
def test_knobs_from_env(mod):
    O, _ = mod
    d = O.OptKnobs.from_env({})
    assert d == O.OptKnobs()
    assert (d.lazy_min_params, d.auto_table_update, d.early_blocks, d.tail_blocks) == (1 << 22, "lazy_exact", 0, 1 << 20)
    assert (d.one_launch, d.variant, d.opt_u, d.scatter_old) == (False, 0, None, False)
    for var, val, field, want in (("MMLREC_LAZY_MIN_PARAMS", "1", "lazy_min_params", 1),
                                  ("MMLREC_AUTO_TABLE_UPDATE", "dense_exact", "auto_table_update", "dense_exact"),
                                  ("MMLREC_EARLY_BLOCKS", "512", "early_blocks", 512),
                                  ("MMLREC_TAIL_BLOCKS", "0", "tail_blocks", 0),
                                  ("MMLREC_OPT_ONE_LAUNCH", "1", "one_launch", True),
                                  ("MMLREC_OPT_VARIANT", "2", "variant", 2),
                                  ("MMLREC_OPT_U", "4", "opt_u", 4),
                                  ("MMLREC_SCATTER_OLD", "1", "scatter_old", True)):
        k = O.OptKnobs.from_env({var: val})
        assert getattr(k, field) == want
        assert k == O.OptKnobs(**{field: want})  # and nothing else moves
    assert O.OptKnobs.from_env({"MMLREC_OPT_ONE_LAUNCH": "0"}).one_launch is False
    assert O.OptKnobs.from_env({"MMLREC_SCATTER_OLD": ""}).scatter_old is False


def test_knobs_read_the_process_environment(mod, monkeypatch):
    O, _ = mod
    monkeypatch.setenv("MMLREC_TAIL_BLOCKS", "3072")
    monkeypatch.delenv("MMLREC_OPT_U", raising=False)
    k = O.OptKnobs.from_env()
    assert (k.tail_blocks, k.opt_u) == (3072, None)
