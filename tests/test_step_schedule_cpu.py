"""The trainer's composition rules, which need no GPU: whole_step_calls (the one-list step and the fork / join inside it),
segmented_step (the two-stream lists), StepKnobs.from_env and the cache key of BaseModel.train_step_runner.  The builders
only look at the entries' kind (E.PY or not), their integer arguments and their meta, so stand-in calls with distinct
tags serve; every expectation is the formula of the builders' docstrings written out."""
import types

import pytest

KNOB_VARS = ("MMLREC_STREAMS", "MMLREC_GRAD_MARKS", "MMLREC_SCATTER_OLD", "MMLREC_MERGE_REDUCES", "MMLREC_MERGE_WGRAD",
             "MMLREC_CU_TAIL", "MMLREC_CU_EARLY", "MMLREC_INNER_FORK", "MMLREC_FORK_MLP", "MMLREC_EARLY_WGRAD",
             "MMLREC_EARLY_WGRAD_DEBUG")
PTR = 0x7f0000100000


@pytest.fixture()
def env():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import engine as E, trainer
    return E, trainer


def f(*a):
    return 0


def c(tag, *args, **meta):
    return (f, (tag,) + args, meta)


def lists(n, tag, **kw):
    return [c("%s%d" % (tag, i), **kw) for i in range(n)]


def make(E, head_side=1, n_pre=0, ready=(1, 2, 3)):
    p = types.SimpleNamespace(fwd=lists(6, "fwd"), head_train=lists(1, "head"), bwd=lists(4, "bwd"),
                              bwd_tail=lists(2, "scatter"), head_side=lists(head_side, "head_side"),
                              bwd_side=[c("wgrad%d" % i, ready=r) for i, r in enumerate(ready)], n_pre=n_pre)
    opt = dict(pre=lists(1, "opt_pre"), early=lists(1, "opt_early"), mlp=lists(2, "opt_mlp"), tables=lists(2, "opt_tab"))
    ar = [(E.PY, f, (), dict(kernel="all_reduce"))]
    return p, opt, ar


FORK, JOIN = ("FORK",), ("JOIN",)


def whole(trainer, p, opt, ar, placement, **kw):
    forked = []

    def make_fork(side):
        forked.append(list(side))
        return FORK, JOIN
    calls, refused = trainer.whole_step_calls(p, opt, ar, placement, make_fork=make_fork, **kw)
    assert len(forked) <= 1
    return calls, refused, (forked[0] if forked else None)


def unforked(p, opt, ar):
    return (opt["pre"] + p.fwd + p.head_train + p.bwd + p.bwd_tail + opt["tables"] + p.head_side + p.bwd_side + ar +
            opt["mlp"])


# ---- the whole-step builder -----------------------------------------------------------------------------------------
def test_whole_step_unforked(env):
    E, trainer = env
    p, opt, ar = make(E)
    for a in ([], ar):
        assert whole(trainer, p, opt, a, 0) == (unforked(p, opt, a), [], None)


@pytest.mark.parametrize("placement", [1, 2, 3])
def test_whole_step_placements(env, placement):
    E, trainer = env
    p, opt, ar = make(E)
    lead = opt["pre"] + p.fwd + p.head_train + p.bwd
    mid = {1: [FORK] + p.bwd_tail + [JOIN] + opt["tables"],
           2: [FORK] + p.bwd_tail + opt["tables"] + [JOIN],
           3: p.bwd_tail + [FORK] + opt["tables"] + [JOIN]}[placement]
    for a in ([], ar):  # (the all-reduce is behind the join: it does not keep the step from forking)
        calls, refused, side = whole(trainer, p, opt, a, placement)
        assert calls == lead + mid + a + opt["mlp"]
        assert refused == [] and side == p.head_side + p.bwd_side


def test_whole_step_fork_mlp(env):
    E, trainer = env
    p, opt, ar = make(E)
    lead = opt["pre"] + p.fwd + p.head_train + p.bwd
    mid = [FORK] + p.bwd_tail + opt["tables"] + [JOIN]
    calls, refused, side = whole(trainer, p, opt, [], 2, fork_mlp=True)
    assert calls == lead + mid and refused == [] and side == p.head_side + p.bwd_side + opt["mlp"]
    calls, refused, side = whole(trainer, p, opt, ar, 2, fork_mlp=True)  # an all-reduce: the MLP update waits for it
    assert calls == lead + mid + ar + opt["mlp"] and refused == [] and side == p.head_side + p.bwd_side
    assert whole(trainer, p, opt, [], 0, fork_mlp=True) == (unforked(p, opt, []), [], None)  # (no fork: nothing moves)


def test_whole_step_empty_head_side(env):
    E, trainer = env
    p, opt, ar = make(E, head_side=0)
    calls, refused, side = whole(trainer, p, opt, [], 2)
    assert side == p.bwd_side and refused == []
    assert calls == (opt["pre"] + p.fwd + p.head_train + p.bwd + [FORK] + p.bwd_tail + opt["tables"] + [JOIN] +
                     opt["mlp"])
    assert whole(trainer, p, opt, [], 0) == (unforked(p, opt, []), [], None)


# ---- the fork predicate -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reason", ["placement", "no_side", "py_side", "py_tail", "py_tables"])
def test_fork_not_taken_without_conflict_list(env, reason):
    E, trainer = env
    p, opt, ar = make(E)
    py = (E.PY, f, ("collective",), {})
    placement = 2
    if reason == "placement":
        placement = 0
    elif reason == "no_side":
        p.head_side, p.bwd_side = [], []
    elif reason == "py_side":
        p.bwd_side.insert(1, py)
    elif reason == "py_tail":
        p.bwd_tail.append(py)
    else:
        opt["tables"].insert(0, py)
    # (a pointer both branches name: the conflict list would not be empty had it been computed)
    if reason != "no_side":
        p.bwd_side.append(c("shared", PTR))
    p.bwd_tail.append(c("shared too", PTR))
    assert whole(trainer, p, opt, [], placement) == (unforked(p, opt, []), [], None)


def test_fork_refused_on_common_pointer_and_shared_scratch(env):
    E, trainer = env
    p, opt, ar = make(E)
    p.bwd_side.append(c("reads", PTR))
    opt["tables"].append(c("writes", PTR))
    for placement in (1, 2, 3):
        assert whole(trainer, p, opt, [], placement) == (unforked(p, opt, []), [PTR], None)
    p, opt, ar = make(E)
    p.bwd_tail.append(c("row kernel", PTR + 0x1000))  # one branch names the shared scratch
    assert whole(trainer, p, opt, [], 2, shared_scratch=[PTR + 0x1000]) == (unforked(p, opt, []), [PTR + 0x1000], None)
    assert whole(trainer, p, opt, [], 2, shared_scratch=[PTR + 0x2000])[2] == p.head_side + p.bwd_side
    p.head_side.append(c("head reduce", ptrs=[PTR + 0x1000]))  # (a buffer named in the meta counts as well)
    assert whole(trainer, p, opt, [], 2) == (unforked(p, opt, []), [PTR + 0x1000], None)


# ---- the segmented builder --------------------------------------------------------------------------------------------
def seg_calls(seg):
    return None if seg is None else [x for kind, item, _ in seg.parts for x in (item if kind == "c" else [item])]


def segmented(trainer, p, opt, ar, wait=(), split=False, marks_rows=False, k=0):
    segs = trainer.segmented_step(p, opt, ar, list(wait), split, marks_rows, k, use_graph=False)
    assert tuple(segs) == trainer.SEGMENT_NAMES
    assert {n: s.min_calls for n, s in segs.items() if s is not None} == {
        n: (1 if n in ("early", "front_b", "side_a") else 2) for n, s in segs.items() if s is not None}
    return {n: seg_calls(s) for n, s in segs.items()}


def test_segmented_unsplit(env):
    E, trainer = env
    p, opt, ar = make(E, n_pre=2)
    for marks_rows in (False, True):  # (neither the marking gather nor n_pre cuts anything off an unsplit step)
        assert segmented(trainer, p, opt, ar, marks_rows=marks_rows) == dict(
            pre=[], early=opt["early"], front=opt["pre"] + p.fwd + p.head_train + p.bwd, front_b=None, side_a=None,
            sideq=p.head_side + p.bwd_side + ar + opt["mlp"], tail=p.bwd_tail + opt["tables"])


@pytest.mark.parametrize("marks_rows", [False, True])
@pytest.mark.parametrize("n_pre", [0, 2])
def test_segmented_split_lead(env, marks_rows, n_pre):
    E, trainer = env
    p, opt, ar = make(E, n_pre=n_pre)
    n_lead = (2 if marks_rows else 0) + n_pre
    wait = [(E.PY, f, (), dict(kernel="wait"))]
    for w in ([], wait):  # (`wait` is in the tail only when the early pass has a stream of its own)
        assert segmented(trainer, p, opt, [], wait=w, split=True, marks_rows=marks_rows) == dict(
            pre=opt["pre"] + p.fwd[:n_lead], early=opt["early"], front=p.fwd[n_lead:] + p.head_train + p.bwd,
            front_b=None, side_a=None, sideq=p.head_side + p.bwd_side + opt["mlp"], tail=p.bwd_tail + w + opt["tables"])


def test_segmented_early_fork(env):
    E, trainer = env
    p, opt, ar = make(E, ready=(1, 2, 3))
    got = segmented(trainer, p, opt, ar, k=0)
    assert got["front_b"] is None and got["side_a"] is None
    assert got["sideq"] == p.head_side + p.bwd_side + ar + opt["mlp"]
    got = segmented(trainer, p, opt, ar, k=2)
    assert got == dict(pre=[], early=opt["early"], front=opt["pre"] + p.fwd + p.head_train + p.bwd[:2], front_b=p.bwd[2:],
                       side_a=p.bwd_side[:2], sideq=p.head_side + p.bwd_side[2:] + ar + opt["mlp"],
                       tail=p.bwd_tail + opt["tables"])


def test_wait_only_with_an_early_stream(env):
    E, trainer = env
    entry = (E.PY, f, (), dict(kernel="wait"))
    for overlap in (False, True):
        for split in (False, True):
            own, wait = trainer.early_stream_wait(overlap, split, entry)
            assert own is (overlap and split) and wait == ([entry] if overlap and split else [])
            p, opt, ar = make(E)
            tail = segmented(trainer, p, opt, [], wait=wait, split=split)["tail"]
            assert tail == p.bwd_tail + ([entry] if overlap and split else []) + opt["tables"]


# ---- the knobs --------------------------------------------------------------------------------------------------------
def test_knobs_defaults(env, monkeypatch):
    E, trainer = env
    for v in KNOB_VARS:
        monkeypatch.delenv(v, raising=False)
    k = trainer.StepKnobs.from_env()
    assert k == trainer.StepKnobs()
    assert (k.streams, k.grad_marks, k.merge_reduces, k.merge_wgrad) == (1, True, True, True)
    assert (k.inner_fork, k.fork_mlp, k.early_wgrad, k.early_wgrad_debug, k.cu_tail, k.cu_early) == (None, False, "0", False, 0, 0)
    assert [k.fork_placement(B) for B in (4096, 16383, 16384, 65536)] == [0, 0, 2, 2]
    assert trainer.resolve_overlap(None) is False and trainer.resolve_overlap(True) is True


@pytest.mark.parametrize("var, value, field, want", [
    ("MMLREC_STREAMS", "2", "streams", 2), ("MMLREC_GRAD_MARKS", "0", "grad_marks", False),
    ("MMLREC_SCATTER_OLD", "1", "grad_marks", False), ("MMLREC_MERGE_REDUCES", "0", "merge_reduces", False),
    ("MMLREC_MERGE_WGRAD", "0", "merge_wgrad", False), ("MMLREC_CU_TAIL", "96", "cu_tail", 96),
    ("MMLREC_CU_EARLY", "32", "cu_early", 32), ("MMLREC_INNER_FORK", "0", "inner_fork", 0),
    ("MMLREC_INNER_FORK", "3", "inner_fork", 3), ("MMLREC_FORK_MLP", "1", "fork_mlp", True),
    ("MMLREC_EARLY_WGRAD", "auto", "early_wgrad", "auto"), ("MMLREC_EARLY_WGRAD", "3", "early_wgrad", "3"),
    ("MMLREC_EARLY_WGRAD_DEBUG", "1", "early_wgrad_debug", True)])
def test_knobs_each_variable(env, monkeypatch, var, value, field, want):
    import dataclasses
    E, trainer = env
    for v in KNOB_VARS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv(var, value)
    k = trainer.StepKnobs.from_env()
    assert getattr(k, field) == want and type(getattr(k, field)) is type(want)
    assert k == dataclasses.replace(trainer.StepKnobs(), **{field: want})  # (and no other field moved)
    if var == "MMLREC_STREAMS":
        assert trainer.resolve_overlap(None) is True and trainer.resolve_overlap(False) is False
    if var == "MMLREC_INNER_FORK":
        assert k.fork_placement(4096) == k.fork_placement(65536) == want


def test_knobs_read_per_construction_and_early_wgrad_index(env, monkeypatch):
    E, trainer = env
    p, opt, ar = make(E)
    monkeypatch.setenv("MMLREC_EARLY_WGRAD", "3")
    k3 = trainer.StepKnobs.from_env()
    monkeypatch.setenv("MMLREC_EARLY_WGRAD", "9")
    k9 = trainer.StepKnobs.from_env()
    monkeypatch.delenv("MMLREC_EARLY_WGRAD")
    assert trainer._early_fork(k3, p, opt["tables"], 65536) == 3      # "3" is the index 3 ...
    assert trainer._early_fork(k9, p, opt["tables"], 65536) == len(p.bwd) - 1   # ... clamped into the chain
    assert trainer._early_fork(trainer.StepKnobs.from_env(), p, opt["tables"], 65536) == 0
    with pytest.raises(Exception):
        k3.early_wgrad = "0"  # frozen


# ---- the cache key of train_step_runner ---------------------------------------------------------------------------------
def test_train_step_runner_caches_by_request(env, monkeypatch):
    E, trainer = env
    from mmlrec_amd.model.basemodel import BaseModel
    for v in KNOB_VARS:
        monkeypatch.delenv(v, raising=False)
    store = object()
    model = types.SimpleNamespace(training=True, use_hip_graph=False, _caches=dict(steps={}), _store=lambda: store)
    built = []

    class Recorder:
        def __init__(self, model, B, use_graph=True, allreduce=None, overlap=None, split_dense=True):
            built.append((B, overlap, split_dense))
            self.store = model._store()
            self.want_overlap, self.want_split = overlap, split_dense
            self.overlap, self.split_dense = False, False  # (what a small row-wise or PCGrad step makes of any request)

    monkeypatch.setattr(trainer, "TrainStep", Recorder)

    def runner(**kw):
        return BaseModel.train_step_runner(model, 4096, **kw)

    a = runner(overlap=True)
    assert runner(overlap=True) is a and built == [(4096, True, True)]
    b = runner(overlap=True, split_dense="force")
    assert b is not a and runner(overlap=True, split_dense="force") is b
    c_ = runner(overlap=True, split_dense=True)
    assert c_ is not b and runner(overlap=True) is c_
    d = runner(overlap=True, split_dense=False)
    assert d is not c_ and runner(overlap=True, split_dense=False) is d
    e = runner()  # (None resolves to one stream: another request than overlap=True)
    assert e is not d and runner(overlap=False, split_dense=True) is e
    assert built == [(4096, True, True), (4096, True, "force"), (4096, True, True), (4096, True, False),
                     (4096, False, True)]
