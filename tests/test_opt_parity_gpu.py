"""The optimizer kernels of csrc/optim.hip against float64 torch.optim on the CPU (tests/opt_refs.py, proved by
tests/test_opt_refs_cpu.py): the flat kernel, the streaming kernel (tail, unaligned fallback, regulariser on marked
launches), the split dense update, the row kernel and the catch-up kernel.

Every comparison is on the UPDATE (after - before, the kernel's own before) and on the state tensors.  The allowance is
measured per case, not fixed: the same inputs go through the reference in float32 and float64, e32 = max |upd32 - upd64|
is what an honest float32 implementation loses, and the kernel gets 4 e32 per element, floored at two spacings of the
value (opt_refs.allowance).  Each case prints `RATIO <case> <kernel's worst error / e32>`.  The catch-up cases use the
bounds of test_lazy_exact_optimizer_matches_dense_trajectory, per group of rows with the same gap."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import opt_refs as R  # noqa: E402

LR = 0.01
REGS = {"none": (0.0, 0.0), "l2": (0.0, 1e-2), "l1": (1e-2, 0.0), "both": (1e-2, 1e-2)}
CUSTOM = dict(betas=(0.8, 0.95), eps=1e-6, alpha=0.9)
F64 = np.float64


def dev():
    return torch.device("cuda:0")


def T(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev())


def host(t):
    return None if t is None else t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import ops as o
    return o


def make_hyper(ops, kind, step=1, step_dev=None, zero_grad=False, max_blocks=0, custom=False):
    h = ops.make_hyper(kind, LR, step=step, step_dev=step_dev, zero_grad=zero_grad, max_blocks=max_blocks)
    if custom:
        h.beta1, h.beta2 = CUSTOM["betas"]
        h.eps, h.alpha = CUSTOM["eps"], CUSTOM["alpha"]
    return h


def step_dense(ops, entries, hyper, empty=()):
    """ops.opt_step_dense, with the descriptors listed in `empty` made zero-length (n = 0 over valid pointers)."""
    from mmlrec_amd import _lib as L
    arr = ops.make_opt_tensors(entries)
    for i in empty:
        arr[i].n = 0
    L.check(L.load().mml_opt_step_dense(arr, len(entries), C.byref(hyper), ops._stream()), "mml_opt_step_dense")


def flat_alloc(n, off):
    """n zeros on the device; off: a [1:] view of n + 1 (the pointer is 4 bytes past a 16-byte boundary)."""
    return torch.zeros(n + 1, device=dev())[1:] if off else torch.zeros(n, device=dev())


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def check_step(tag, got, before, ref, ref_before, e32):
    """got = (p, s1, s2) of the kernel after the step (float32 host arrays or None), before = its p before; ref /
    ref_before the float64 reference's.  Returns the worst error / e32 over p and the states."""
    ratios = [R.assert_within(tag + " update", got[0].astype(F64) - before.astype(F64), ref[0] - ref_before, e32[0],
                              before)]
    for i in (1, 2):
        if ref[i] is not None:
            ratios.append(R.assert_within(f"{tag} state{i}", got[i], ref[i], e32[i], ref[i]))
    return max(ratios)


def say(case, ratio):
    print(f"RATIO {case} {ratio:.2f}")


# ---- flat kernel -----------------------------------------------------------------------------------------------------
# 1, 7, 1023, 4096 elements, a zero-length descriptor (over a 4-element buffer that must not move) and a [1:] view of a
# 1025-element buffer (scalar path); 40 tensors in one call = two launches (MML_MAX_OPT_TENSORS = 32)
FLAT_SIZES = [1, 7, 1023, 4096, 0, -1024]
FLAT_CASES = [(k, r, "host_step") for k in R.KINDS for r in REGS] + \
             [(k, "both", m) for k in R.KINDS for m in ("custom", "step_dev")]


@functools.lru_cache(maxsize=1)
def flat_inputs():
    """(sizes, buffer lengths, offsets, zero-length descriptors, p0, grads, live elements) of the 40 tensors, as one flat
    array each; the buffers behind the zero-length descriptors hold 1.25 / 0.5 and are not `live`."""
    rng = np.random.default_rng(31)
    sizes = [FLAT_SIZES[i % len(FLAT_SIZES)] for i in range(40)]
    lens = [abs(s) if s else 4 for s in sizes]
    off = np.concatenate([[0], np.cumsum(lens)])
    empty = [i for i, s in enumerate(sizes) if s == 0]
    p0, grads = R.draw_inputs(rng, int(off[-1]), 4)
    live = np.ones(off[-1], bool)
    for i in empty:
        live[off[i]:off[i + 1]] = False
        p0[off[i]:off[i + 1]] = 1.25
        for g in grads:
            g[off[i]:off[i + 1]] = 0.5
    for a in [p0, live] + grads:
        a.setflags(write=False)
    return sizes, lens, off, empty, p0, grads, live


def flat_reference(kind, reg, custom):
    _, _, _, _, p0, grads, live = flat_inputs()
    l1, l2 = REGS[reg]
    return R.reference_case(kind, p0[live], [g[live] for g in grads], lr=LR, l1=l1, l2=l2, **(CUSTOM if custom else {}))


@pytest.mark.parametrize("kind,reg,mode", FLAT_CASES)
def test_flat_kernel(ops, kind, reg, mode):
    steps = 4
    sizes, lens, off, empty, p0, grads, live = flat_inputs()
    l1, l2 = REGS[reg]
    tr64, e32 = flat_reference(kind, reg, mode == "custom")
    dead = p0[live] == 0
    assert dead.any() and not dead.all()

    def alloc(src=None):
        ts = [flat_alloc(n, s < 0) for n, s in zip(lens, sizes)]
        if src is not None:
            for i, t in enumerate(ts):
                t.copy_(T(src[off[i]:off[i + 1]]))
        return ts

    def cat(ts):
        return np.concatenate([host(t) for t in ts])

    tp, tg = alloc(p0), alloc()
    ts1 = alloc() if kind != "sgd" else None
    ts2 = alloc() if kind == "adam" else None
    assert tp[5].data_ptr() % 16 == 4 and tp[3].data_ptr() % 16 == 0
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev())
    before, ref_before = p0.copy(), p0[live].astype(F64)
    worst = 0.0
    for k in range(steps):
        for i, t in enumerate(tg):
            t.copy_(T(grads[k][off[i]:off[i + 1]]))
        if mode == "step_dev":
            ops.counter_update(step_dev, 1)
            hyper = make_hyper(ops, kind, step=0, step_dev=step_dev, zero_grad=True)
        else:
            hyper = make_hyper(ops, kind, step=k + 1, zero_grad=True, custom=mode == "custom")
        step_dense(ops, [(tp[i], tg[i], ts1[i] if ts1 else None, ts2[i] if ts2 else None, (l1, l2))
                         for i in range(len(sizes))], hyper, empty=empty)
        p, g = cat(tp), cat(tg)
        s1, s2 = (cat(ts1) if ts1 else None), (cat(ts2) if ts2 else None)
        tag = f"flat {kind} {reg} {mode} step {k + 1}"
        worst = max(worst, check_step(tag, (p[live], s1[live] if ts1 else None, s2[live] if ts2 else None),
                                      before[live], tr64[k], ref_before, e32[k]))
        assert not p[live][dead].any(), tag + ": an element with p = 0 and g = 0 moved"
        assert not g[live].any(), tag + ": zero_grad left a gradient"
        # the zero-length descriptors' buffers are untouched
        assert np.array_equal(p[~live], p0[~live]) and np.array_equal(g[~live], grads[k][~live])
        assert (s1 is None or not s1[~live].any()) and (s2 is None or not s2[~live].any())
        before, ref_before = p, tr64[k][0]
    say(f"flat/{kind}/{reg}/{mode}", worst)


# ---- streaming kernel, unmarked --------------------------------------------------------------------------------------
N_STREAM = (1 << 24) + 3     # n % 4 == 3: the scalar tail behind the vector loop


@functools.lru_cache(maxsize=1)
def stream_reference(kind, reg):
    """(p0, grads, float64 trajectory, e32) of the streaming cases of one (kind, regulariser): shared by the aligned and
    the offset tensor and both grids, read-only."""
    rng = np.random.default_rng(41)
    p0, grads = R.draw_inputs(rng, N_STREAM, 2)
    l1, l2 = REGS[reg]
    tr64, e32 = R.reference_case(kind, p0, grads, lr=LR, l1=l1, l2=l2)
    for a in [p0] + grads + [x for st in tr64 for x in st if x is not None]:
        a.setflags(write=False)
    return p0, grads, tr64, e32


STREAM_CASES = [(k, r, v, mb) for k in ("adam", "sgd") for r in ("none", "both") for v in (False, True)
                for mb in (0, 300)]


@pytest.mark.parametrize("kind,reg,view,max_blocks", STREAM_CASES)
def test_streaming_kernel_unmarked(ops, kind, reg, view, max_blocks):
    """One tensor of 2^24 + 3 elements through opt_dense_kernel: 16-byte aligned (vector loop + scalar tail) and as a
    [1:] view (every element through the fallback loop), full grid and 300 workgroups."""
    p0, grads, tr64, e32 = stream_reference(kind, reg)
    l1, l2 = REGS[reg]
    dead = p0 == 0
    tp, tg = flat_alloc(N_STREAM, view), flat_alloc(N_STREAM, view)
    ts1 = flat_alloc(N_STREAM, view) if kind == "adam" else None
    ts2 = flat_alloc(N_STREAM, view) if kind == "adam" else None
    tp.copy_(T(p0))
    assert tp.data_ptr() % 16 == (4 if view else 0)
    before, ref_before = p0, p0.astype(F64)
    worst = 0.0
    for k in range(2):
        tg.copy_(T(grads[k]))
        step_dense(ops, [(tp, tg, ts1, ts2, (l1, l2))],
                   make_hyper(ops, kind, step=k + 1, zero_grad=True, max_blocks=max_blocks))
        p = host(tp)
        tag = f"stream {kind} {reg} view={view} max_blocks={max_blocks} step {k + 1}"
        worst = max(worst, check_step(tag, (p, host(ts1), host(ts2)), before, tr64[k], ref_before, e32[k]))
        assert not p[dead].any(), tag + ": an element with p = 0 and g = 0 moved"
        assert float(tg.abs().max()) == 0.0, tag + ": zero_grad left a gradient"
        before, ref_before = p, tr64[k][0]
    say(f"stream/{kind}/{reg}/{'offset' if view else 'aligned'}/{max_blocks}", worst)


# ---- split dense update ----------------------------------------------------------------------------------------------
def row_bitmap(mask):
    """bool [V] -> int32 words on the device, bit (row & 31) of word (row >> 5)."""
    pad = np.zeros((len(mask) + 31) // 32 * 32, bool)
    pad[:len(mask)] = mask
    return T(np.packbits(pad, bitorder="little").view(np.int32))


def start_state(rng, kind, shape):
    """Moments as a few steps of gradients leave them (float32): Adam m, v | RMSprop square_avg."""
    g = rng.standard_normal(shape)
    if kind == "adam":
        return (0.1 * g).astype(np.float32), (1e-3 * g * g + 1e-6).astype(np.float32)
    return (1e-2 * g * g + 1e-6).astype(np.float32), None


@functools.lru_cache(maxsize=1)
def split_case(kind, E, big):
    """One dense step (number 3) from given moments, the gradient zero outside the rows of the bitmap: rows 0 and V - 1
    set, word 2 all ones, word 3 all zeros, 1 % of the others."""
    V = (1 << 24) // E + 37 if big else 1000
    assert V % 32 != 0
    rng = np.random.default_rng(51)
    p0, (g,) = R.draw_inputs(rng, (V, E), 1, zero_share=0.0, grad_share=1.0)
    s1, s2 = start_state(rng, kind, (V, E))
    mask = rng.random(V) < 0.01
    mask[[0, V - 1]] = True
    mask[64:96], mask[96:128] = True, False
    g[~mask] = 0.0
    tr = [[R.masked_step(kind, p0, s1, s2, g, None, 3, lr=LR, dtype=dt)] for dt in (torch.float32, torch.float64)]
    e32 = R.e32_of(tr[0], tr[1], p0)[0]
    for a in (p0, s1, s2, g, mask) + tr[1][0]:
        if a is not None:
            a.setflags(write=False)
    return p0, s1, s2, g, mask, tr[1][0], e32


SPLIT_CASES = [(k, E, big, mb) for k in ("adam", "rmsprop") for E in (4, 16) for big in (True, False)
               for mb in (0, 512)]


@pytest.mark.parametrize("kind,E,big,max_blocks", SPLIT_CASES)
def test_split_update(ops, kind, E, big, max_blocks):
    """mml_opt_tensor.skip_rows with zero_grads, then mml_opt_step_rows over the set rows: together one dense step.
    big: V E >= 2^24 (opt_dense_kernel: OPT_PLAIN, under max_blocks OPT_SKIP_U); else the flat kernel."""
    p0, s1_0, s2_0, g, mask, ref, e32 = split_case(kind, E, big)
    V = p0.shape[0]
    md = torch.from_numpy(mask.copy()).to(dev())
    tp, ts1 = T(p0), T(s1_0)
    ts2 = T(s2_0) if s2_0 is not None else None
    tg = T(g)
    tg[~md] = float("nan")        # zero_grads: the gradient of an unset row is not read
    seen = row_bitmap(mask)
    tag = f"split {kind} E={E} V={V} max_blocks={max_blocks}"
    step_dense(ops, [(tp, tg, ts1, ts2, None, seen)], make_hyper(ops, kind, step=3, zero_grad=True,
                                                                  max_blocks=max_blocks))
    for t, t0 in ((tp, p0), (ts1, s1_0), (ts2, s2_0)):
        if t is not None:
            assert same_bits(t[md], T(t0)[md]), tag + ": the early launch touched a set row"
            assert not torch.isnan(t).any(), tag + ": a gradient that must not be read was read"
    assert torch.isnan(tg[~md]).all() and same_bits(tg[md], T(g)[md]), tag + ": the early launch wrote gradients"
    assert (host(ts1)[~mask] != s1_0[~mask]).all(), tag + ": the early launch left an unset row's state"
    rows = np.flatnonzero(mask).astype(np.int32)
    ops.opt_step_rows([tp], [tg], [ts1], [ts2] if ts2 is not None else None, [seen], [0, V], T(rows),
                      T(np.array([len(rows)], np.int32)), make_hyper(ops, kind, step=3))
    ratio = check_step(tag, (host(tp), host(ts1), host(ts2)), p0, ref, p0.astype(F64), e32)
    assert int(seen.abs().max()) == 0 and float(tg[md].abs().max()) == 0.0 and torch.isnan(tg[~md]).all()
    say(f"split/{kind}/E{E}/{'stream' if big else 'flat'}/{max_blocks}", ratio)


# ---- marked launch with a regulariser --------------------------------------------------------------------------------
MARK_E = 8
MARK_VOCAB = {"one": [(1 << 24) // MARK_E + 5], "seven": [(1 << 24) // MARK_E + 5, 1, 37, 300000, 4097, 64, 250001]}


@functools.lru_cache(maxsize=1)
def marked_case(which):
    """Two Adam steps with l2 = 1e-2 over tables whose gradient is non-zero on the rows of a 3 000-sample batch only."""
    vocab = MARK_VOCAB[which]
    rb = np.concatenate([[0], np.cumsum(vocab)])
    rng = np.random.default_rng(61)
    p0, _ = R.draw_inputs(rng, (int(rb[-1]), MARK_E), 0)
    Xs, hits, grads = [], [], []
    for _ in range(2):
        X = np.stack([np.r_[0, v - 1, rng.integers(0, v, 2998)] for v in vocab], 1)
        hit = np.zeros(rb[-1], bool)
        for f in range(len(vocab)):
            hit[rb[f] + X[:, f]] = True
        g = np.zeros_like(p0)
        g[hit] = rng.standard_normal((int(hit.sum()), MARK_E)).astype(np.float32)
        g[p0 == 0] = 0.0
        Xs.append(X.astype(np.float32))
        hits.append(hit)
        grads.append(g)
    tr64, e32 = R.reference_case("adam", p0, grads, lr=LR, l2=1e-2)
    return p0, Xs, hits, grads, tr64, e32


@pytest.mark.parametrize("which,max_blocks", [(w, mb) for w in ("one", "seven") for mb in (0, 300)])
def test_marked_launch_with_regulariser(ops, which, max_blocks):
    """grad_marks with l2: an unmarked row still moves, by the l2 term alone, and its gradient (NaN here) is not read."""
    p0, Xs, hits, grads, tr64, e32 = marked_case(which)
    vocab = MARK_VOCAB[which]
    F, E = len(vocab), MARK_E
    rb = np.concatenate([[0], np.cumsum(vocab)])
    base = np.concatenate([[0], np.cumsum([(v + 31) // 32 * 32 for v in vocab])]).tolist()
    tabs = [T(p0[rb[f]:rb[f + 1]]) for f in range(F)]
    tm = [torch.zeros(v, E, device=dev()) for v in vocab]
    tv = [torch.zeros(v, E, device=dev()) for v in vocab]
    tg = [torch.zeros(v, E, device=dev()) for v in vocab]
    marks = torch.zeros(ops.marks_bytes(vocab), dtype=torch.uint8, device=dev())
    rng = np.random.default_rng(62)
    dead = p0 == 0

    def cat(ts):
        return np.concatenate([host(t) for t in ts])

    before, ref_before = p0, p0.astype(F64)
    worst = 0.0
    for k in range(2):
        tag = f"marked {which} max_blocks={max_blocks} step {k + 1}"
        # the marks come from the scatter; the gradient itself from the host (the same bits for both grids), NaN where
        # the row is unmarked
        ops.scatter_bwd(tg, T(Xs[k]), list(range(F)), T(rng.standard_normal((3000, F * E)).astype(np.float32)),
                        marks=marks)
        for f in range(F):
            got = host(marks[base[f]:base[f] + vocab[f]]).astype(bool)
            assert np.array_equal(got, hits[k][rb[f]:rb[f + 1]]), tag
            g = grads[k][rb[f]:rb[f + 1]].copy()
            g[~hits[k][rb[f]:rb[f + 1]]] = np.nan
            tg[f].copy_(T(g))
        step_dense(ops, [(tabs[f], tg[f], tm[f], tv[f], (0.0, 1e-2), None, marks[base[f]:base[f] + vocab[f]])
                         for f in range(F)], make_hyper(ops, "adam", step=k + 1, zero_grad=True, max_blocks=max_blocks))
        p, m, v, g = cat(tabs), cat(tm), cat(tv), cat(tg)
        assert not (np.isnan(p).any() or np.isnan(m).any() or np.isnan(v).any()), tag + ": an unmarked gradient was read"
        worst = max(worst, check_step(tag, (p, m, v), before, tr64[k], ref_before, e32[k]))
        assert not p[dead].any(), tag
        assert int(marks.max()) == 0, tag + ": marks not cleared"
        assert not g[hits[k]].any() and np.isnan(g[~hits[k]]).all(), tag
        for t in tg:
            t.zero_()
        before, ref_before = p, tr64[k][0]
    say(f"marked/{which}/{max_blocks}", worst)


# ---- row kernel ------------------------------------------------------------------------------------------------------
ROW_VARIANTS = {"E5": (5, False), "E8": (8, False), "E12": (12, False), "E8_offset": (8, True)}


@pytest.mark.parametrize("variant", list(ROW_VARIANTS))
@pytest.mark.parametrize("kind", R.KINDS)
def test_row_kernel(ops, kind, variant):
    """mml_opt_step_rows = the dense step restricted to the listed rows, the others and their state frozen.  E = 5
    and a table 4 bytes off alignment take opt_rows_kernel<1>, E = 8 and 12 opt_rows_kernel<4>; the count word says
    more rows than the list holds; `last` gets the step of the device counter."""
    E, offset = ROW_VARIANTS[variant]
    vocab, steps = [50, 3000], 3
    rb = [0, 50, 3050]
    rng = np.random.default_rng(71)
    p0, grads = R.draw_inputs(rng, (rb[-1], E), steps, grad_share=0.8)
    lists, masks = [], []
    for _ in range(steps):
        rows = np.unique(np.r_[0, 49, 50, 3049, rng.integers(0, rb[-1], 300)])
        lists.append(rng.permutation(rows).astype(np.int32))
        mask = np.zeros(rb[-1], bool)
        mask[rows] = True
        masks.append(mask)
    tr64 = R.masked_trajectory(kind, p0, grads, masks, lr=LR)
    tr32 = R.masked_trajectory(kind, p0, grads, masks, lr=LR, dtype=torch.float32)
    e32 = R.e32_of(tr32, tr64, p0)
    dead = p0 == 0

    def alloc(f, src=None):
        n = vocab[f] * E
        t = flat_alloc(n, offset and f == 1).view(vocab[f], E)
        if src is not None:
            t.copy_(T(src[rb[f]:rb[f + 1]]))
        return t

    def cat(ts):
        return np.concatenate([host(t) for t in ts])

    tabs = [alloc(f, p0) for f in range(2)]
    tg = [alloc(f) for f in range(2)]
    ts1 = [alloc(f) for f in range(2)] if kind != "sgd" else None
    ts2 = [alloc(f) for f in range(2)] if kind == "adam" else None
    assert tabs[1].data_ptr() % 16 == (4 if offset else 0)
    last = [torch.full((v,), -5, dtype=torch.int32, device=dev()) for v in vocab]
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev())
    before, ref_before = p0, p0.astype(F64)
    s_before = [None, None]
    want_last = np.full(rb[-1], -5)
    worst = 0.0
    for k in range(steps):
        tag = f"rows {kind} {variant} step {k + 1}"
        mask = masks[k]
        extra = (np.arange(rb[-1]) % 7 == 3) & ~mask          # `seen` bits of rows that are not listed: they stay
        seen = [row_bitmap((mask | extra)[rb[f]:rb[f + 1]]) for f in range(2)]
        g = grads[k].copy()
        g[~mask] = np.nan
        for f in range(2):
            tg[f].copy_(T(g[rb[f]:rb[f + 1]]))
        touched = T(lists[k])
        count = T(np.array([len(lists[k]) + 7], np.int32))    # more than the list's capacity: the kernel stops at it
        ops.counter_update(step_dev, 1)
        ops.opt_step_rows(tabs, tg, ts1, ts2, seen, rb, touched, count,
                          make_hyper(ops, kind, step=0, step_dev=step_dev), last=last)
        p = cat(tabs)
        s = [cat(ts1) if ts1 else None, cat(ts2) if ts2 else None]
        worst = max(worst, check_step(tag, (p, s[0], s[1]), before, tr64[k], ref_before, e32[k]))
        assert np.array_equal(p[~mask].view(np.int32), before[~mask].view(np.int32)), tag + ": an unlisted row moved"
        for a, b in zip(s, s_before):
            if a is not None and b is not None:
                assert np.array_equal(a[~mask].view(np.int32), b[~mask].view(np.int32)), tag + ": unlisted state moved"
        assert not p[dead].any(), tag
        gg = cat(tg)
        assert not gg[mask].any() and np.isnan(gg[~mask]).all(), tag + ": gradients"
        for f in range(2):
            assert torch.equal(seen[f], row_bitmap(extra[rb[f]:rb[f + 1]])), tag + ": seen bits"
        want_last[mask] = k + 1
        assert np.array_equal(cat(last), want_last), tag + ": last"
        before, ref_before, s_before = p, tr64[k][0], s
    say(f"rows/{kind}/{variant}", worst)


# ---- catch-up --------------------------------------------------------------------------------------------------------
def catchup_state(rng, kind, shape):
    p, _ = R.draw_inputs(rng, shape, 0, zero_share=0.0)
    m, v = start_state(rng, kind, shape)
    return p, m, v


def check_catchup(tag, kind, got, before, frm, target):
    """got / before = (p, m, v) of the rows caught up from step frm[row] to target, against the float64 replay; per
    group of rows with the same gap: p within 2e-6 max|p| + 1e-9 and the moments within 2e-5 of their largest, as
    test_lazy_exact_optimizer_matches_dense_trajectory has them; a gap above 45 steps gets 4 e32 of the float32 replay
    where that is more."""
    ref = R.zero_grad_replay(kind, *before, frm, target, lr=LR)
    r32 = R.zero_grad_replay(kind, *before, frm, target, lr=LR, dtype=np.float32)
    for gap in np.unique(target - frm):
        rows = (target - frm) == gap
        names = ("p", "state1", "state2")
        for i in range(3):
            if ref[i] is None:
                continue
            a, b = got[i][rows].astype(F64), ref[i][rows]
            scale = np.abs(b).max()
            bound = 2e-6 * scale + 1e-9 if i == 0 else 2e-5 * scale
            e32 = float(np.abs(r32[i][rows].astype(F64) - b).max())
            if gap > 45:
                bound = max(bound, 4 * e32)
            err = np.abs(a - b).max()
            assert err <= bound, f"{tag} gap {gap} {names[i]}: error {err:.3e}, bound {bound:.3e}, e32 {e32:.3e}"
        if gap == 0:
            for i in range(3):
                if before[i] is not None:
                    assert np.array_equal(got[i][rows].view(np.int32), before[i][rows].view(np.int32)), \
                        tag + ": a current row changed"
    return ref


@pytest.mark.parametrize("target", [40, 200])
@pytest.mark.parametrize("E", [5, 12, 16])
@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_catchup_rows(ops, kind, E, target):
    """300 listed rows over 3 tables, `last` = target (nothing to do), target - 1, target - 30 and 0 (target 200: the
    early exit once p stops moving); a fifth of the rows with m = 0 (Adam: p stays, v decays)."""
    vocab = [40, 600, 2000]
    rb = np.concatenate([[0], np.cumsum(vocab)]).tolist()
    rng = np.random.default_rng(81)
    p, m, v = catchup_state(rng, kind, (rb[-1], E))
    rows = rng.permutation(np.unique(np.r_[0, rb[-1] - 1, rng.choice(rb[-1], 320, replace=False)])[:300])
    frm_all = rng.integers(0, target + 1, rb[-1])
    frm_all[rows] = np.array([target, target - 1, 0, target - 30])[np.arange(len(rows)) % 4]
    still = rows[np.arange(len(rows)) % 5 == 0]
    m[still] = 0.0
    tabs = [T(p[rb[f]:rb[f + 1]]) for f in range(3)]
    tm = [T(m[rb[f]:rb[f + 1]]) for f in range(3)]
    tv = [T(v[rb[f]:rb[f + 1]]) for f in range(3)] if kind == "adam" else None
    last = [T(frm_all[rb[f]:rb[f + 1]].astype(np.int32)) for f in range(3)]
    ops.opt_catchup_rows(tabs, tm, tv, last, rb, T(rows.astype(np.int32)), T(np.array([len(rows)], np.int32)),
                         make_hyper(ops, kind, step=target + 1))

    def cat(ts):
        return None if ts is None else np.concatenate([host(t) for t in ts])

    got = (cat(tabs), cat(tm), cat(tv))
    tag = f"catchup rows {kind} E={E} target={target}"
    listed = np.zeros(rb[-1], bool)
    listed[rows] = True
    for a, b in zip(got, (p, m, v)):
        if a is not None:
            assert np.array_equal(a[~listed].view(np.int32), b[~listed].view(np.int32)), tag + ": an unlisted row changed"
    want_last = frm_all.copy()
    want_last[rows] = target
    assert np.array_equal(cat(last), want_last), tag + ": last"
    sel = lambda t: tuple(None if a is None else a[rows] for a in t)  # noqa: E731
    check_catchup(tag, kind, sel(got), sel((p, m, v)), frm_all[rows], target)
    assert np.array_equal(got[0][still].view(np.int32), p[still].view(np.int32)), tag + ": p moved with m = 0"
    if kind == "rmsprop":
        assert np.array_equal(got[0].view(np.int32), p.view(np.int32)), tag + ": RMSprop moved p without a gradient"
    moved = np.setdiff1d(rows[frm_all[rows] < target], still)
    decayed, was = (got[2], v) if kind == "adam" else (got[1], m)
    assert (decayed[moved] != was[moved]).all(), tag + ": a listed row behind the target kept its state"


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_catchup_dense_row_dealt_across_two_grid_passes(ops, kind):
    """V = 45 000, E = 12: 540 000 elements against a grid of 2 048 x 256 lanes.  Dealt as row * E + e, row 43 690 owns
    items 524 280 .. 524 291 -- elements 0 - 7 with the last lanes of the last workgroup's first pass, elements 8 - 11
    with the first lanes of workgroup 0's second pass, which then found last[row] already published and skipped them.
    The rows of workgroup 0's first pass replay 40 steps, so that its second pass comes late."""
    V, E, target = 45000, 12, 40
    row = (2048 * 256) // E
    assert row * E < 2048 * 256 < (row + 1) * E - 3
    rng = np.random.default_rng(91)
    p, m, v = catchup_state(rng, kind, (V, E))
    m[row] = 0.1 if kind == "adam" else 0.01
    frm = rng.choice([target, target - 1, target - 5], V)
    frm[:(256 + E - 1) // E] = 0
    frm[row] = target - 1
    tp, tm = T(p), T(m)
    tv = T(v) if kind == "adam" else None
    last = T(frm.astype(np.int32))
    ops.opt_catchup_dense(tp, tm, tv, last, make_hyper(ops, kind, step=target))
    got = (host(tp), host(tm), host(tv))
    tag = f"catchup dense {kind}"
    assert int(last.min()) == target and int(last.max()) == target, tag + ": last"
    # every element of the straddling row decayed its first moment / square average, and Adam moved p
    assert (got[1][row] != m[row]).all(), tag + f": row {row} elements {np.flatnonzero(got[1][row] == m[row])} skipped"
    if kind == "adam":
        assert (got[0][row] != p[row]).all(), tag
    check_catchup(tag, kind, got, (p, m, v), frm, target)


def test_catchup_refuses_rows_wider_than_a_wave(ops):
    from mmlrec_amd import _lib as L
    t = [torch.zeros(4, 65, device=dev()) for _ in range(3)]
    last = torch.zeros(4, dtype=torch.int32, device=dev())
    with pytest.raises(L.MMLError):
        ops.opt_catchup_dense(t[0], t[1], t[2], last, make_hyper(ops, "adam", step=3))
    assert not t[0].any() and not last.any()
