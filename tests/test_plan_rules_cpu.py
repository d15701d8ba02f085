"""The rules inside the call-list passes (passes.py) and around them, which need no GPU: reindex_ready, slab_cost /
wgrad_chunks / targets_distinct, match_tower_head, the fused-plan guard, Plan.prepend with the two prologues, and
PlanKnobs.from_env.  Stand-in functions and ctypes descriptors as in test_plan_passes_cpu.py; every expectation is
written out by hand from the passes' docstrings."""
import ctypes as C
import dataclasses
import types

import pytest

PLAN_VARS = ("MMLREC_AMAX", "MMLREC_BF16_STORAGE", "MMLREC_GEMM_PLANES", "MMLREC_MERGE_COPIES", "MMLREC_AMAX_MERGE",
             "MMLREC_NT_GROUP", "MMLREC_TOWER_HEAD", "MMLREC_GATHER_WGMAX", "MMLREC_DET_FUSED", "MMLREC_GRAD_PARTS",
             "MMLREC_GRAD_COLS", "MMLREC_SPLIT_DGRAD")


@pytest.fixture()
def env():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, engine as E, passes as P
    return L, E, P


def fn(name):
    def f(*a):
        return 0
    f.__name__ = name
    return f


def side(ready):
    return (fn("wgrad"), (ready,), dict(side=True, ready=ready))


# ---- reindex_ready ------------------------------------------------------------------------------------------------------
def test_reindex_ready_after_a_merge(env):
    """Seven old entries into five (1 + 2 and 4 + 5 merged).  ready = k becomes where[k - 1] + 1; 0 stays 0; a tag at the
    end of the chain becomes the merged chain's length."""
    L, E, P = env
    where = [0, 1, 1, 2, 3, 3, 4]
    calls = [side(k) for k in (0, 1, 2, 3, 4, 5, 6, 7)]
    untagged = (fn("copy"), (0,), dict(side=True))
    P.reindex_ready(calls + [untagged], where)
    assert [c[2]["ready"] for c in calls] == [0, 1, 2, 2, 3, 4, 4, 5]
    assert "ready" not in untagged[2]


@pytest.mark.parametrize("di", [0, 2, 5])
def test_reindex_ready_after_one_deletion(env, di):
    """fuse_tower_head's table for deleting bwd[di] of six entries: tags <= di stay, tags > di drop by one (ready == di
    and ready == di + 1 both end at di)."""
    L, E, P = env
    n = 6
    where = list(range(di)) + [P.DELETED] + list(range(di, n - 1))
    assert len(where) == n
    calls = [side(k) for k in range(n + 1)]
    P.reindex_ready(calls, where)
    assert [c[2]["ready"] for c in calls] == [k - 1 if k > di else k for k in range(n + 1)]
    by_hand = {0: [0, 0, 1, 2, 3, 4, 5], 2: [0, 1, 2, 2, 3, 4, 5], 5: [0, 1, 2, 3, 4, 5, 5]}
    assert [c[2]["ready"] for c in calls] == by_hand[di]


# ---- the weight-gradient tile model -------------------------------------------------------------------------------------
def test_slab_cost_recorded_cases(env):
    """merge_wgrad's recorded cases at B = 65 536 (2 048 steps of 32 rows; divisor 8, cap 64), each + 8 for the launch +
    reduction pair; merge_wgrad16's KuaiRec-32 case (1 024 steps of 64 rows; divisor 4, cap 32)."""
    L, E, P = env
    steps = 65536 // 32
    assert [P.slab_cost(t, steps, 8, 64) for t in (20, 8, 2)] == [82 + 8, 32 + 8, 32 + 8]       # AE-30, per layer
    assert P.slab_cost(30, steps, 8, 64) == 121 + 8                                             # ... merged
    assert [P.slab_cost(t, steps, 8, 64) for t in (72, 32, 4)] == [293 + 8, 128 + 8, 32 + 8]    # KuaiRec-32, per layer
    assert P.slab_cost(108, steps, 8, 64) == 512 + 8                                            # ... merged
    s16 = 65536 // 64
    # towers (4 tiles: 32 slabs of 32 steps) + second expert layers (32 tiles: 16 slabs of 64 steps) against 36 tiles
    # (14 slabs of 74 steps)
    assert (P.slab_cost(4, s16, 4, 32), P.slab_cost(32, s16, 4, 32), P.slab_cost(36, s16, 4, 32)) == (32 + 8, 64 + 8, 74 + 8)
    assert P.slab_cost(36, s16, 4, 32) < P.slab_cost(4, s16, 4, 32) + P.slab_cost(32, s16, 4, 32)   # -> one launch


def test_wgrad_chunks_recorded_cases(env):
    L, E, P = env
    B = 65536
    ae30 = [[(512, 640)], [(256, 512)], [(128, 256)]]        # 4 x 5 = 20, 2 x 4 = 8, 1 x 2 = 2 tiles
    assert P.wgrad_chunks(ae30, [True] * 3, B, L.NT_MAX_GROUP) == [[0, 1, 2]]     # 90 + 40 + 40 against 129: merge
    kuairec = [[(1024, 1152)], [(512, 1024)], [(256, 256)]]  # 8 x 9 = 72, 4 x 8 = 32, 2 x 2 = 4 tiles
    assert P.wgrad_chunks(kuairec, [True] * 3, B, L.NT_MAX_GROUP) is None         # 301 + 136 + 40 against 520: per layer
    # a tile count is rounded UP per problem: 129 x 1 output elements are two tiles
    assert P.wgrad_chunks([[(512, 640)], [(256, 512)], [(129, 1)]], [True] * 3, B, L.NT_MAX_GROUP) == [[0, 1, 2]]
    # a problem the kernel's predicate declines goes into a launch of its own kind, behind the others
    # (22 tiles: 90 + 8 steps, 8 tiles: 32 + 8, against 170 per layer)
    assert P.wgrad_chunks(ae30, [True, False, True], B, L.NT_MAX_GROUP) == [[0, 2], [1]]
    # nt_group cuts what the predicate takes into launches of even size
    five = [[(128, 128)] for _ in range(5)]
    assert P.wgrad_chunks(five, [True] * 5, B, 2) == [[0, 1], [2, 3], [4]]        # 3 x 40 against 5 x 40
    assert P.wgrad_chunks(five, [True] * 5, B, 1) is None                         # one problem per launch: nothing won


def test_targets_distinct(env):
    L, E, P = env

    def descs(*rows):
        out = []
        for dW, dbias, acc in rows:
            d = L.GemmWgradDesc()
            d.dW, d.dbias, d.accumulate = dW, dbias, acc
            out.append(d)
        return out

    assert P.targets_distinct(descs((0x1000, 0x2000, 0), (0x3000, 0, 0), (0x4000, 0, 0)))   # (no bias: no target)
    assert not P.targets_distinct(descs((0x1000, 0x2000, 0), (0x1000, 0x3000, 0)))          # a shared dW
    assert not P.targets_distinct(descs((0x1000, 0x2000, 0), (0x3000, 0x2000, 0)))          # a shared dbias
    assert not P.targets_distinct(descs((0x1000, 0x2000, 0), (0x3000, 0x4000, 1)))          # somebody accumulates
    g16 = L.G16WgradDesc()
    g16.dW, g16.dbias = 0x1000, 0x2000
    assert P.targets_distinct([g16])


# ---- match_tower_head ---------------------------------------------------------------------------------------------------
def tower_pattern(L, tweak=None):
    """The smallest lists fuse_tower_head takes: T = 2 towers of 48 -> 32 columns over 64 rows.  tweak(parts) edits the
    descriptors / lists before they are matched."""
    lib = types.SimpleNamespace(mml_head_bce_fwd_bwd_phase=fn("head"), mml_gemm_grouped_fwd=fn("fwd"),
                                mml_gemm_grouped_dgrad=fn("dgrad"), other=fn("other"))
    grp = L.HeadGroup()
    grp.n_heads, grp.B, grp.y, grp.prob, grp.loss = 2, 64, 0x1000, 0x2000, 0x3000
    farr, darr = (L.GemmFwdDesc * 2)(), (L.GemmDgradDesc * 2)()
    for t in range(2):
        h = grp.head[t]
        h.Hin, h.dH, h.w, h.bias, h.dw, h.dbias = (0x10000 * (k + 1) + 0x1000 * t for k in range(6))
        h.ldh, h.lddh, h.H, h.h_relu = 32, 32, 32, 1
        f = farr[1 - t]  # (the forward launch lists the towers in the other order: matched by pointer, not by position)
        f.A, f.W, f.bias, f.C = 0x100000 + t, 0x200000 + 0x1000 * t, 0x300000 + t, h.Hin
        f.lda, f.ldw, f.ldc, f.M, f.N, f.K, f.act = 48, 48, 32, 64, 32, 48, L.ACT_RELU
        f.amax_a, f.w_planes, f.w_kexp = 0x400000, 0x500000 + t, 0x600000 + t
        d = darr[t]
        d.dA, d.ldda, d.M, d.K, d.act, d.n_src = 0x700000 + t, 48, 64, 48, L.ACT_NONE, 1
        d.dC[0], d.W[0], d.lddc[0], d.ldw[0], d.N[0] = h.dH, f.W, 32, 32, 32
        d.w_planes[0], d.w_kexp[0] = 0x800000 + t, 0x900000 + t
    parts = types.SimpleNamespace(
        lib=lib, grp=grp, farr=farr, darr=darr,
        fwd=[(lib.other, (0,)), (lib.mml_gemm_grouped_fwd, (farr, 2), dict(kernel="gemm<fwd>"))],
        head_train=[(lib.mml_head_bce_fwd_bwd_phase, (C.byref(grp), 0xa00000, 256, 1), dict(kernel="head"))],
        head_side=[(lib.mml_head_bce_fwd_bwd_phase, (C.byref(grp), 0xa00000, 256, 2), dict(side=True, ready=0))],
        bwd=[(lib.other, (1,)), (lib.mml_gemm_grouped_dgrad, (darr, 2), dict(kernel="gemm<dgrad>")), (lib.other, (2,))])
    if tweak is not None:
        tweak(parts)
    return parts


def matched(P, p):
    return P.match_tower_head(p.fwd, p.head_train, p.head_side, p.bwd, p.lib)


def test_match_tower_head_takes_the_pattern(env):
    L, E, P = env
    p = tower_pattern(L)
    fi, di, tasks = matched(P, p)
    assert (fi, di, len(tasks)) == (1, 1, 2)
    for t, (f, d, h) in enumerate(tasks):
        assert h.Hin == p.grp.head[t].Hin and f.C == h.Hin and d.dC[0] == h.dH and d.W[0] == f.W
    g = P.build_tower_head(p.grp, tasks)
    assert (g.n, g.M, g.y, g.prob, g.loss) == (2, 64, 0x1000, 0x2000, 0x3000)
    for t in range(2):
        q, (f, d, h) = g.t[t], tasks[t]
        assert (q.A, q.K, q.N, q.w_planes_fwd, q.w_planes_bwd) == (f.A, 48, 32, f.w_planes, d.w_planes[0])
        assert (q.dH, q.dA, q.dw, q.dhbias, q.head) == (h.dH, d.dA, h.dw, h.dbias, t)


def _two_head_calls(p):
    p.head_train = p.head_train * 2


@pytest.mark.parametrize("tweak", [
    lambda p: setattr(p.grp.head[1], "gate", 0xb00000),           # a head with a gate
    lambda p: setattr(p.farr[0], "C", 0xc00000),                  # a forward problem whose C is not a head's Hin
    lambda p: setattr(p.darr[0], "n_src", 2),                     # a dgrad with two sources
    lambda p: p.darr[1].W.__setitem__(0, 0xd00000),               # W differs between forward and dgrad
    lambda p: setattr(p.farr[1], "ldc", 36),                      # ldc != ldh
    _two_head_calls,                                              # two head_train entries
], ids=["gated_head", "foreign_C", "two_sources", "W_mismatch", "ldc_ne_ldh", "two_head_calls"])
def test_match_tower_head_refuses(env, tweak):
    L, E, P = env
    assert matched(P, tower_pattern(L)) is not None
    assert matched(P, tower_pattern(L, tweak)) is None


# ---- the fused-plan guard -----------------------------------------------------------------------------------
def test_fused_plan_refuses_the_entry_points_that_read_the_heads_input(env):
    import torch
    L, E, P = env
    plan = E.Plan(torch.device("cpu"), 4, True)
    plan.run_forward()              # (empty lists: nothing to run)
    plan.run_backward_from_dprob()
    plan.tower_head = L.TowerHeadGroup()   # what passes.fuse_tower_head leaves on success
    for entry in (plan.run_forward, plan.run_backward_from_dprob):
        with pytest.raises(L.MMLError, match="fuse_tower_head"):
            entry()
    plan.run_train_fwd_bwd()


# ---- Plan.prepend and the prologues -------------------------------------------------------------------------------------
def prologue_plan(L, E, amax_merge):
    import torch
    lib = types.SimpleNamespace(**{n: fn(n) for n in (
        "mml_amax_reset", "mml_amax_batch", "mml_gemm_planes_cut", "mml_gemm_grouped_fwd", "mml_pep_gate_fwd",
        "mml_cast16_batch", "mml_gather_fwd", "mml_counter_update", "mml_copy2d")})
    plan = E.Plan(torch.device("cpu"), 4, True)
    plan.knobs = dataclasses.replace(plan.knobs, amax_merge=amax_merge)
    plan.amax_pool = torch.zeros(8, 8, dtype=torch.int32)   # (a CPU plan has no pool of its own)
    plan.amax_next = 3
    x, w = torch.zeros(4, 16), torch.zeros(8, 16)
    plan.amax_wlist = [(w, plan.amax_pool[1])]
    plan.cast16_items = [(w, torch.zeros(8, 16, dtype=torch.bfloat16), False)]
    plan.fwd = [(lib.mml_gather_fwd, (0,), dict(kernel="gather")),
                plan.amax_call([(x, plan.amax_pool[0])], lib=lib, tag="input"),
                (lib.mml_gemm_grouped_fwd, (0, 1), dict(kernel="gemm<fwd>"))]
    return lib, plan


def names(calls):
    return [c[0].__name__ for c in calls]


@pytest.mark.parametrize("amax_merge", [True, False])
def test_prepend_keeps_n_pre_and_the_order(env, amax_merge):
    L, E, P = env
    lib, plan = prologue_plan(L, E, amax_merge)
    body = ["mml_gather_fwd", "mml_amax_batch", "mml_gemm_grouped_fwd"]
    # Plan.finish's order: magnitudes, then the cast launch in front of them
    P.amax_prologue(plan, lib=lib)
    amax_pre = ["mml_amax_reset"] if amax_merge else ["mml_amax_reset", "mml_amax_batch"]
    assert names(plan.fwd) == amax_pre + body and plan.n_pre == len(amax_pre)
    host = plan.fwd[plan.n_pre + 1]
    # merged: the weights ride in the input's launch, which keeps its own tags
    assert len(host[2]["need"]) == (2 if amax_merge else 1) and host[1][1] == len(host[2]["need"]) and host[2]["tag"] == "input"
    P.cast16_prologue(plan, lib=lib)
    assert names(plan.fwd) == ["mml_cast16_batch"] + amax_pre + body and plan.n_pre == 1 + len(amax_pre)
    # the step counter of an uncompiled model with dropout (BaseModel._finish_record): positions 0 and 1
    plan.prepend([(lib.mml_counter_update, (0, 1, 0)), (lib.mml_copy2d, (0, 1, 0, 1, 1, 1, 0))])
    want = ["mml_counter_update", "mml_copy2d", "mml_cast16_batch"] + amax_pre + body
    assert names(plan.fwd) == want and plan.n_pre == 3 + len(amax_pre)
    assert names(plan.fwd[plan.n_pre:]) == body
    # a prologue that already ran adds nothing
    P.amax_prologue(plan, lib=lib)
    P.cast16_prologue(plan, lib=lib)
    assert names(plan.fwd) == want and plan.n_pre == 3 + len(amax_pre)


def test_prologues_without_work_leave_the_plan_alone(env):
    import torch
    L, E, P = env
    lib = types.SimpleNamespace()  # (no function is looked up)
    plan = E.Plan(torch.device("cpu"), 4, True)
    P.amax_prologue(plan, lib=lib)
    P.cast16_prologue(plan, lib=lib)
    assert plan.fwd == [] and plan.n_pre == 0 and not plan.amax_pre_done and not plan.cast16_pre_done


# ---- PlanKnobs ----------------------------------------------------------------------------------------------------------
def test_plan_knobs_defaults(env, monkeypatch):
    L, E, P = env
    for v in PLAN_VARS:
        monkeypatch.delenv(v, raising=False)
    k = E.PlanKnobs.from_env()
    assert k == E.PlanKnobs() and k == E.PlanKnobs.from_env({})
    assert (k.amax, k.nt_group) == (None, L.NT_MAX_GROUP)
    assert all(getattr(k, f.name) is True for f in dataclasses.fields(k) if f.name not in ("amax", "nt_group"))
    assert len(dataclasses.fields(k)) == len(PLAN_VARS)


@pytest.mark.parametrize("var, value, field, want", [
    ("MMLREC_AMAX", "0", "amax", False), ("MMLREC_AMAX", "1", "amax", True),
    ("MMLREC_BF16_STORAGE", "0", "bf16_storage", False), ("MMLREC_GEMM_PLANES", "0", "gemm_planes", False),
    ("MMLREC_MERGE_COPIES", "0", "merge_copies", False), ("MMLREC_AMAX_MERGE", "0", "amax_merge", False),
    ("MMLREC_NT_GROUP", "16", "nt_group", 16), ("MMLREC_NT_GROUP", "0", "nt_group", 1),
    ("MMLREC_TOWER_HEAD", "0", "tower_head", False), ("MMLREC_GATHER_WGMAX", "0", "gather_wgmax", False),
    ("MMLREC_DET_FUSED", "0", "det_fused", False), ("MMLREC_GRAD_PARTS", "0", "grad_parts", False),
    ("MMLREC_GRAD_COLS", "0", "grad_cols", False), ("MMLREC_SPLIT_DGRAD", "0", "split_dgrad", False)])
def test_plan_knobs_each_variable(env, monkeypatch, var, value, field, want):
    import torch
    L, E, P = env
    for v in PLAN_VARS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv(var, value)
    k = E.PlanKnobs.from_env()
    assert getattr(k, field) == want and type(getattr(k, field)) is type(want)
    assert k == dataclasses.replace(E.PlanKnobs(), **{field: want})  # (and no other field moved)
    plan = E.Plan(torch.device("cpu"), 4, True)   # read once per construction, kept on the plan
    assert plan.knobs == k
    monkeypatch.delenv(var)
    assert plan.knobs == k and E.Plan(torch.device("cpu"), 4, True).knobs == E.PlanKnobs()


def test_plan_knobs_amax_decides_by_batch_when_unset(env, monkeypatch):
    import torch
    L, E, P = env
    monkeypatch.delenv("MMLREC_AMAX", raising=False)
    cpu = torch.device("cpu")
    assert [E.Plan(cpu, B, True).use_amax for B in (4096, 32767, 32768, 65536)] == [False, False, True, True]
    monkeypatch.setenv("MMLREC_AMAX", "1")
    assert E.Plan(cpu, 4096, True).use_amax and not E.Plan(cpu, 65536, True, use_amax=False).use_amax
    monkeypatch.setenv("MMLREC_AMAX", "0")
    assert not E.Plan(cpu, 65536, True).use_amax
    monkeypatch.setenv("MMLREC_NT_GROUP", "1000")
    assert E.PlanKnobs.from_env().nt_group == L.NT_MAX_GROUP   # (never more than one launch takes)
