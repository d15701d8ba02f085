"""mml_opt_step_dense's launch rule (csrc/opt_plan.hpp: kernel, grid, OptLaunch.variant / .prop / .blk0 of one group of
tensors) off the GPU.  tests/opt_plan_driver.cpp, a stand-alone program around the header, is compiled with g++ and fed
cases; every expected plan below is the rule of the header worked out by hand for 256 compute units and the default knobs
(variant 0, cold_wgs 2 048, resident_per_cu 8, u_mark 2).  The Python mirrors of the rule (_lib.opt_dense_streams,
optimizer.opt_dense_symbol) are held against the same program."""
import functools
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT
from test_optimizer_plan_cpu import AE30_ROWS

E8 = 8
BIG = [10_000_000, 1_000_000, 1_000_000]
ALL30 = AE30_ROWS[3:] + AE30_ROWS[:3]  # small tables first, as the step lists them
SMALL27 = AE30_ROWS[3:]
CAP = 1 << 20
ENV = dict(cus=256, variant=0, cold_wgs=2048, per_cu=8, u_mark=2)
_tmp = None


@functools.lru_cache(maxsize=None)
def driver():
    """The compiled driver (once per session, in a temporary directory that lives as long as the process)."""
    global _tmp
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import build
    _tmp = tempfile.TemporaryDirectory()
    exe = os.path.join(_tmp.name, "opt_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", build.CSRC,
                           os.path.join(ROOT, "tests", "opt_plan_driver.cpp"), "-o", exe])
    return exe


def tensors(rows, marks=True, warm=False, acc=False, skip=False, E=E8):
    """[rows, E] tables as the driver's tensor tuples; the map pointers are distinct 64-byte aligned numbers."""
    return [(r * E, E, (1 << 20) + 64 * k if marks else 0, (1 << 21) + 64 * k if warm else 0,
             (1 << 22) + 64 * k if acc else 0, (1 << 23) + 64 * k if skip else 0) for k, r in enumerate(rows)]


def run_plans(cases):
    """cases: (tensor tuples, max_blocks, cold_loop, knobs) -> one parsed plan each: ("flat", grid.x), ("refused", message)
    or a dict with form, U, grid, prop, variant, blk0."""
    text = ""
    for ts, max_blocks, cold_loop, knobs in cases:
        k = dict(ENV, **knobs)
        text += "%d %d %d %d %d %d %d %d" % (k["cus"], k["variant"], k["cold_wgs"], k["per_cu"], k["u_mark"], max_blocks,
                                             cold_loop, len(ts))
        text += "".join(" %d %d %d %d %d %d" % t for t in ts) + "\n"
    lines = subprocess.run([driver()], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(cases), lines
    out = []
    for ln in lines:
        w = ln.split()
        if w[0] == "flat":
            out.append(("flat", int(w[1])))
        elif w[0] == "refused":
            out.append(("refused", ln[len("refused "):]))
        else:
            assert [w[0], w[2], w[4], w[7], w[9], w[11]] == ["form", "U", "grid", "prop", "variant", "blk0"], ln
            out.append(dict(form=int(w[1]), U=int(w[3]), grid=(int(w[5]), int(w[6])), prop=int(w[8]), variant=int(w[10]),
                            blk0=[int(x) for x in w[12:]]))
    return out


def one(ts, max_blocks=CAP, cold_loop=0, **knobs):
    return run_plans([(ts, max_blocks, cold_loop, knobs)])[0]


def brief(p):
    return (p["form"], p["U"], p["grid"], p["prop"])


# ---- the table of plans ---------------------------------------------------------------------------------------------
def test_big_tables():
    assert [r * E8 for r in BIG] == [80_000_000, 8_000_000, 8_000_000]
    p = one(tensors(BIG))
    assert brief(p) == (3, 2, (2048, 3), 0) and p["variant"] == 4 and p["blk0"] == []
    warm = tensors(BIG, warm=True)
    p = one(warm, cold_loop=0)
    assert brief(p) == (3, 2, (2048, 1), 2) and p["blk0"] == [0, 39063, 42970, 46877]
    assert brief(one(warm, cold_loop=3)) == (3, 2, (1024, 1), 2)
    p = one(warm, cold_loop=2)
    assert brief(p) == (3, 2, (2048, 3), 0) and p["variant"] == 4
    p = one(warm, cold_loop=1)
    assert brief(p) == (3, 2, (2048, 3), 0) and p["variant"] == 12
    odd = list(warm)
    odd[1] = odd[1][:3] + (odd[1][3] + 1,) + odd[1][4:]  # one warm map at an odd address: not resident
    assert brief(one(odd, cold_loop=0)) == (3, 2, (2048, 3), 0)
    odd[1] = warm[1][:2] + (warm[1][2] + 2,) + warm[1][3:]  # (or a mark map that is only 2-byte aligned)
    assert brief(one(odd, cold_loop=0)) == (3, 2, (2048, 3), 0)


def test_big_tables_capped():
    warm = tensors(BIG, warm=True)
    assert brief(one(warm, 300, cold_loop=2)) == (3, 2, (100, 3), 0)
    assert brief(one(warm, 300, cold_loop=0)) == (3, 2, (300, 1), 2)
    assert brief(one(warm, 1, cold_loop=0)) == (3, 2, (3, 1), 2)
    # neither capped nor deferred: the plain loop, which has no resident grid
    p = one(warm, 0, cold_loop=0)
    assert brief(p) == (0, 1, (2048, 3), 0) and p["variant"] == 0


def test_all_30_with_totals():
    assert len(ALL30) == 30 and sum(r * E8 for r in SMALL27) == 3_908_816
    ts = tensors(ALL30, warm=True, acc=True)
    p = one(ts, 0, cold_loop=0)
    assert brief(p) == (4, 2, (2048, 1), 2) and p["blk0"][30] == 48800 and p["blk0"][0] == 0
    p = one(ts, 0, cold_loop=2)
    assert brief(p) == (4, 2, (9975, 1), 1) and p["blk0"][30] == 9975
    # above the cap (every tensor is clamped to at least one workgroup): pinned as it is
    assert brief(one(ts, 300, cold_loop=2)) == (4, 2, (319, 1), 1)
    assert brief(one(ts, 300, cold_loop=0)) == (4, 2, (319, 1), 2)
    assert brief(one(ts, 0, cold_loop=0, cus=304)) == (4, 2, (2432, 1), 2)
    unmarked = list(ts)
    unmarked[7] = tensors([ALL30[7]], marks=False)[0]
    kind, msg = one(unmarked, 0)
    assert kind == "refused" and "acc64 tensors takes grad_marks on every tensor" in msg


def test_small_tables_take_the_flat_kernel():
    ts = tensors(SMALL27, marks=False)
    assert one(ts) == ("flat", 2048)
    assert one(ts, 300) == ("flat", 300)
    ts[5] = tensors([SMALL27[5]])[0]
    kind, msg = one(ts)
    assert kind == "refused" and "only honoured by the streaming launch" in msg


def test_unmarked_and_split_forms():
    assert brief(one(tensors(BIG, marks=False), variant=2))[:2] == (1, 1)
    assert brief(one(tensors(BIG, marks=False, skip=True), 512)) == (2, 4, (171, 3), 0)


def test_chunks_in_flight():
    assert [one(tensors(BIG), u_mark=u)["U"] for u in (4, 8, 3)] == [4, 8, 2]
    acc = tensors(ALL30, warm=True, acc=True)
    assert [brief(one(acc, 0, u_mark=u))[:2] for u in (4, 8)] == [(4, 4), (4, 2)]


# ---- the Python mirrors ---------------------------------------------------------------------------------------------
@pytest.fixture()
def mod():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, optimizer as O
    return O, L


STREAMING = [(tensors(BIG), CAP), (tensors(BIG, warm=True), CAP), (tensors(BIG, warm=True), 0),
             (tensors(ALL30, warm=True, acc=True), 0), (tensors(ALL30, warm=True, acc=True), 300),
             (tensors(ALL30), CAP), (tensors(BIG, marks=False), CAP), (tensors(BIG, marks=False), 0),
             (tensors(BIG, marks=False, skip=True), 512), (tensors(BIG, marks=False, skip=True), 0)]


def test_symbol_names_the_planned_instantiation(mod):
    """optimizer.opt_dense_symbol (the label of a call list entry, which profiles are read by) against the C plan, for
    every MMLREC_OPT_U the knobs admit -- one without an instantiation included."""
    O, _ = mod
    for opt_u in (None, 2, 3, 4, 8):
        for variant in (0, 2):
            knobs = dict(variant=variant, **({} if opt_u is None else dict(u_mark=opt_u)))
            plans = run_plans([(ts, cap, 0, knobs) for ts, cap in STREAMING])
            for (ts, cap), p in zip(STREAMING, plans):
                total = sum(t[0] for t in ts)
                assert O.opt_dense_symbol(total, len(ts), p["form"], opt_u) == \
                    "opt_dense_kernel<true, %d, %d>" % (p["form"], p["U"]), (opt_u, variant, cap, len(ts))


def test_streams_mirror(mod):
    O, L = mod
    cases, keys = [], []
    for total in ((1 << 24) - 8, 1 << 24):
        for n in (1, 4, 5, 30):
            for marked in (False, True):
                rows = [total // E8 - (n - 1)] + [1] * (n - 1)
                cases.append((tensors(rows, marks=marked), CAP, 0, {}))
                keys.append((total, n, marked))
    for (total, n, marked), p in zip(keys, run_plans(cases)):
        if marked and not L.opt_dense_streams(total, n, marked):
            assert p[0] == "refused"  # (the flat kernel takes no marks)
        else:
            assert L.opt_dense_streams(total, n, marked) == isinstance(p, dict), (total, n, marked)
        assert (O.opt_dense_symbol(total, n, 3 if marked else 0) == "opt_flat_kernel") == (not isinstance(p, dict))
