"""The marked streaming table update on ONE grid sized for the chip (csrc/optim.hip: cold_resident, mml_opt_hyper.cold_loop
= 0): the 256-row spans of all tensors of the launch form one index space and wave w of the grid takes spans w, w + W, ...;
and the step's constants read from the buffer mml_opt_step_begin fills instead of computed by every workgroup.

Everything is compared bit for bit, in the style and with the helpers of test_opt_cold_compact_gpu.py.  The references of a
resident launch are the same launch with cold_loop = 1 (the byte-walking loop on each tensor's own workgroups) and the
launch without a warm map (every row updated), from the same state and the same gradient bits: p, m, v, the gradient, the
64-bit totals and the marks are equal, the warm map is exactly (old warm OR marked), the canary bytes around the maps and
the two canary rows behind every tensor are untouched.  Two steps in a row.

Which launches take the resident grid: forms 3 (under a workgroup cap) and 4 when every tensor has a warm map at a
4-byte aligned address; form 3 with max_blocks = 0 is launched as the plain loop form and checks that loop against the same
references.  One tensor with an odd map address sends the whole launch to the per-tensor grid (that tensor to the byte
loop), cold_loop = 2 runs the compacted loop on the per-tensor grid, cold_loop = 3 halves the resident grid: all the same
bits, so no case can tell which ran -- that is read from mml_opt_step_dense."""
import functools

import pytest

from test_opt_cold_compact_gpu import CANARY, SMALL, _map_views, _pattern

pytestmark = pytest.mark.gpu

PATTERNS = ("none", "row0", "last", "every257", "span", "all", "rand4", "rand15", "rand70")
MAX_OPT_TENSORS = 32


@pytest.fixture(scope="module")
def env():
    import torch
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, ops
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    assert L.MAX_OPT_TENSORS == MAX_OPT_TENSORS
    return torch, L, ops


def big(E):
    return (1 << 24) // E + 37  # the streaming launch exists from 2^24 parameters up


def layout(E, where):
    """The seven small tables beside the large one: in their middle, first or last."""
    at = {"middle": 3, "first": 0, "last": len(SMALL)}[where]
    return tuple(SMALL[:at]) + (big(E),) + tuple(SMALL[at:])


def counted(E, n):
    """n tensors, small ones (the sizes of SMALL over and over) around large ones.  Every launch of the call must stream
    2^24 parameters: the 33rd tensor is the second launch of its call and is a large table itself."""
    if n == 1:
        return (big(E),)
    v = [SMALL[i % len(SMALL)] for i in range(n)]
    v[min(n, MAX_OPT_TENSORS) // 2] = big(E)
    if n > MAX_OPT_TENSORS:
        v[-1] = big(E)
    return tuple(v)


@functools.lru_cache(maxsize=1)
def _masters(E, vocab):
    """Per (width, tables), built once and never written: the tables' start values and moments for the warm rows."""
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(23 + E + len(vocab))
    p0 = [torch.randn(v + 2, E, generator=g, device=dev) for v in vocab]
    m0 = [torch.randn(v + 2, E, generator=g, device=dev) * 0.1 + 0.01 for v in vocab]
    v0 = [torch.rand(v + 2, E, generator=g, device=dev) + 0.01 for v in vocab]
    return p0, m0, v0


def _run(env, E, form, cap, name, vocab, cold_loop=0, odd_at=None, steps=(1, 2)):
    torch, L, ops = env
    dev = torch.device("cuda:0")
    p0, m0, v0 = _masters(E, vocab)
    F = len(vocab)
    std_base = [0]
    for v in vocab:
        std_base.append(std_base[-1] + (v + 31) // 32 * 32)
    marks_std = torch.zeros(ops.marks_bytes(list(vocab)), dtype=torch.uint8, device=dev)

    def maps():
        """Zeroed views behind canaries; tensor odd_at's view starts one byte behind a multiple of 32, the others on one."""
        buf, views, out = _map_views(torch, vocab, False, dev)
        if odd_at is not None:
            o = views[odd_at].data_ptr() - buf.data_ptr()
            buf[o] = CANARY                                   # (the byte the view gives up; one more canary behind it)
            out[o] = True
            out[o + vocab[odd_at]] = False
            views[odd_at] = buf[o + 1:o + 1 + vocab[odd_at]]
            views[odd_at].zero_()
        return buf, views, out

    # the run under test (A), the byte loop with a map (B), no map (C): marks each, warm maps for A and B
    mbuf, marks, m_out = maps()
    wbuf, warm, w_out = maps()
    _, marks_b, _ = maps()
    _, warm_b, _ = maps()
    _, marks_c, _ = maps()
    for f, v in enumerate(vocab):
        want_odd = 1 if f == odd_at else 0
        assert marks[f].data_ptr() % 4 == want_odd and warm[f].data_ptr() % 4 == want_odd
        assert int(mbuf[marks[f].data_ptr() - mbuf.data_ptr() - 1]) == CANARY          # directly before ...
        assert int(mbuf[marks[f].data_ptr() - mbuf.data_ptr() + v]) == CANARY          # ... and directly after
    warm0 = [_pattern(torch, name, v, 0, dev)[1] for v in vocab]
    full = {"p": [x.clone() for x in p0], "m": [], "v": [], "g": [], "acc": []}
    for f, v in enumerate(vocab):
        keep = torch.cat([warm0[f], torch.ones(2, dtype=torch.bool, device=dev)]).view(-1, 1)
        full["m"].append(torch.where(keep, m0[f], torch.zeros_like(m0[f])))
        full["v"].append(torch.where(keep, v0[f], torch.zeros_like(v0[f])))
        full["g"].append(torch.cat([torch.zeros(v, E, device=dev), torch.full((2, E), 3.0, device=dev)]))
        full["acc"].append(torch.cat([torch.zeros(v, E, dtype=torch.int64, device=dev),
                                      torch.full((2, E), 12345, dtype=torch.int64, device=dev)]))
        warm[f].copy_(warm0[f].to(torch.uint8))
        warm_b[f].copy_(warm[f])
    refs = [{k: [x.clone() for x in xs] for k, xs in full.items()} for _ in range(2)]
    canaries = {k: [x[v:].clone() for x, v in zip(xs, vocab)] for k, xs in full.items()}
    view = lambda d, k: [x[:v] for x, v in zip(d[k], vocab)]  # noqa: E731
    slot = ops.amax_slots(1, dev)[0]
    for step in steps:
        want = [_pattern(torch, name, v, step, dev)[0].nonzero().view(-1) for v in vocab]
        B = max(int(w.numel()) for w in want)
        shift = ops.scatter_det_shift(max(B, 1))
        if B:                                                                    # (a table with no row to mark lends row 0)
            X = torch.stack([torch.cat([w, (w[:1] if w.numel() else w.new_zeros(1)).repeat(B - w.numel())])
                             for w in want], 1).to(torch.float32).contiguous()
            gd = torch.Generator(device=dev).manual_seed(step)
            d = torch.randn(B, F * E, generator=gd, device=dev)
            if form == 4:
                slot.zero_()
                ops.amax_batch([(d, slot)])
                ops.scatter_bwd_det(view(full, "g"), X, list(range(F)), d, view(full, "acc"), marks_std, amax_slot=slot,
                                    clear_marks=False, amax_supplied=True, defer_totals=True)
            else:
                ops.scatter_bwd(view(full, "g"), X, list(range(F)), d, marks=marks_std)
        marked, old_warm = [], []
        for f, v in enumerate(vocab):                                            # the scatter's marks, moved behind canaries
            marks[f].copy_(marks_std[std_base[f]:std_base[f] + v])
            marks_b[f].copy_(marks[f])
            marks_c[f].copy_(marks[f])
            marked.append(marks[f] != 0)
            old_warm.append(warm[f] != 0)
            assert int(marked[f].sum()) >= int(want[f].numel())
            for r in refs:                                                       # the same gradient bits in all runs
                r["g"][f].copy_(full["g"][f])
                r["acc"][f].copy_(full["acc"][f])
        marks_std.zero_()
        det = (lambda d_, f: (d_["acc"][f][:vocab[f]], slot, shift)) if form == 4 else (lambda d_, f: None)
        ent = lambda d_, mk, wm: [(d_["p"][f][:v], d_["g"][f][:v], d_["m"][f][:v], d_["v"][f][:v], None, None, mk[f],  # noqa: E731
                                   det(d_, f), wm[f] if wm else None) for f, v in enumerate(vocab)]
        hyper = lambda loop: ops.make_hyper("adam", 0.01, step=step, zero_grad=True, max_blocks=cap, cold_loop=loop)  # noqa: E731
        ops.opt_step_dense(ent(full, marks, warm), hyper(cold_loop))
        ops.opt_step_dense(ent(refs[0], marks_b, warm_b), hyper(1))
        ops.opt_step_dense(ent(refs[1], marks_c, None), hyper(0))
        for f, v in enumerate(vocab):
            for ref in refs:
                for k in ("p", "m", "v", "g"):
                    assert torch.equal(full[k][f][:v].view(torch.int32), ref[k][f][:v].view(torch.int32)), (k, f, step)
                assert torch.equal(full["acc"][f][:v], ref["acc"][f][:v]), (f, step)
            assert torch.equal(marks[f], marks_c[f]) and int(marks[f].max()) == 0, (f, step)
            assert torch.equal(warm[f], warm_b[f]), (f, step)
            assert torch.equal(warm[f] != 0, old_warm[f] | marked[f]), (f, step)
            assert int(warm[f].max()) <= 1
            assert float(full["g"][f][:v].abs().max()) == 0.0 and int(full["acc"][f][:v].abs().max()) == 0
            for k in full:                                                       # nothing behind the last row moved
                assert torch.equal(full[k][f][v:], canaries[k][f]), (k, f, step)
        for buf, out in ((mbuf, m_out), (wbuf, w_out)):                          # every byte outside the views
            assert bool((buf[out] == CANARY).all()), step
    if name != "none":
        f = vocab.index(big(E))
        assert not torch.equal(full["p"][f], p0[f])                              # (the steps did move something)


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("form", [3, 4])
@pytest.mark.parametrize("E", [4, 8, 16])
def test_patterns(env, E, form, name):
    _run(env, E, form, 300, name, layout(E, "middle"))


@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("form", [3, 4])
@pytest.mark.parametrize("E", [4, 8, 16])
def test_caps(env, E, form, cap):
    """max_blocks = 0 (form 4: the chip-sized grid; form 3: the plain loop form) and 1 (one workgroup per tensor today, so
    eight workgroups for all spans)."""
    _run(env, E, form, cap, "every257", layout(E, "middle"))


@pytest.mark.parametrize("cap", [0, 1, 300])
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("form", [3, 4])
@pytest.mark.parametrize("E", [4, 8, 16])
def test_large_table_first_and_last(env, E, form, where, cap):
    _run(env, E, form, cap, "rand4", layout(E, where))


@pytest.mark.parametrize("n", [1, 2, 8, MAX_OPT_TENSORS, MAX_OPT_TENSORS + 1])
@pytest.mark.parametrize("form", [3, 4])
@pytest.mark.parametrize("E", [4, 8, 16])
def test_tensor_counts(env, E, form, n):
    """1 and 2 tensors (the launch's grid was (workgroups, tensors) before), 8 and the most a launch takes, and one more:
    two launches."""
    _run(env, E, form, 300, "rand15", counted(E, n))


@pytest.mark.parametrize("form", [3, 4])
def test_fewer_spans_than_waves(env, form):
    """One table of 4 097 spans (not a multiple of anything in sight): 2 048 workgroups = 8 192 waves on a 256-CU chip under
    form 4, whose surplus waves leave at once; form 3 keeps its 300 workgroups = 1 200 waves."""
    assert (big(16) + 255) // 256 == 4097
    _run(env, 16, form, 0 if form == 4 else 300, "rand15", (big(16),))


@pytest.mark.parametrize("form", [3, 4])
@pytest.mark.parametrize("E", [4, 8, 16])
def test_halved_grid(env, E, form):
    _run(env, E, form, 0 if form == 4 else 300, "rand4", layout(E, "middle"), cold_loop=3)


@pytest.mark.parametrize("odd_at", [1, 3])
@pytest.mark.parametrize("form", [3, 4])
@pytest.mark.parametrize("E", [4, 8, 16])
def test_one_odd_map_sends_the_launch_back(env, E, form, odd_at):
    """A small table (odd_at = 1) or the large one (3) with maps at an odd address among aligned ones: the launch takes the
    per-tensor grid, that tensor the byte loop."""
    _run(env, E, form, 300, "every257", layout(E, "middle"), odd_at=odd_at)


@pytest.mark.parametrize("name", ["span", "rand4"])
@pytest.mark.parametrize("form", [3, 4])
@pytest.mark.parametrize("E", [4, 8, 16])
def test_per_tensor_arm(env, E, form, name):
    """cold_loop = 2 (MMLREC_OPT_RESIDENT=0): the compacted loop on the workgroups of each tensor."""
    _run(env, E, form, 300, name, layout(E, "middle"), cold_loop=2)


# ---- the step's constants ---------------------------------------------------------------------------------------------
def _dense_case(torch, ops, kind, E, seed):
    """A marked streaming launch (form 3 under a cap, warm maps: the resident grid), a flat launch and a row launch worth
    of state, as dicts of tensors."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    V = big(E)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    st = dict(p=r(V, E), m=r(V, E) * 0.1, v=torch.rand(V, E, generator=g, device=dev), g=r(V, E) * 0.01,
              fp=r(1001), fm=r(1001) * 0.1, fv=torch.rand(1001, generator=g, device=dev), fg=r(1001),
              rp=r(300, E), rm=r(300, E) * 0.1, rv=torch.rand(300, E, generator=g, device=dev), rg=r(300, E))
    if kind != "adam":                                                 # (state1 is a sum of squares there)
        for k in ("m", "fm", "rm"):
            st[k].abs_()
    st["marks"] = (torch.rand(V, generator=g, device=dev) < 0.05).to(torch.uint8)
    st["warm"] = (torch.rand(V, generator=g, device=dev) < 0.5).to(torch.uint8)
    cold = (st["warm"] == 0).view(-1, 1)
    st["m"].masked_fill_(cold, 0.0)
    st["v"].masked_fill_(cold, 0.0)
    st["g"].masked_fill_((st["marks"] == 0).view(-1, 1), 0.0)
    return st


def _three_kernels(torch, ops, kind, st, step_dev, E):
    """opt_dense_kernel, opt_flat_kernel and opt_rows_kernel once each under step_dev."""
    dev = st["p"].device
    s2 = lambda k: st[k] if kind == "adam" else None  # noqa: E731
    s1 = lambda k: st[k] if kind != "sgd" else None  # noqa: E731
    h = ops.make_hyper(kind, 0.01, step=0, step_dev=step_dev, max_blocks=300)
    marks, warm = st["marks"].clone(), st["warm"].clone()
    ops.opt_step_dense([(st["p"], st["g"], s1("m"), s2("v"), None, None, marks, None, warm if kind != "sgd" else None)], h)
    ops.opt_step_dense([(st["fp"], st["fg"], s1("fm"), s2("fv"))], h)
    seen = torch.full(((300 + 31) // 32,), -1, dtype=torch.int32, device=dev)
    touched = torch.arange(0, 300, 3, dtype=torch.int32, device=dev)
    count = torch.tensor([touched.numel()], dtype=torch.int32, device=dev)
    ops.opt_step_rows([st["rp"]], [st["rg"].clone()], [s1("rm")] if kind != "sgd" else None,
                      [s2("rv")] if kind == "adam" else None, [seen], [0, 300], touched, count, h)


def _equal_bits(torch, a, b):
    for k in a:
        x, y = a[k], b[k]
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y), k


@pytest.mark.parametrize("step", [1, 2, 999, 100000])
def test_adam_constants_bound_against_unbound(env, step):
    torch, L, ops = env
    dev = torch.device("cuda:0")
    a, b = _dense_case(torch, ops, "adam", 8, 5), _dense_case(torch, ops, "adam", 8, 5)
    bound, consts = ops.step_counter(dev)
    plain = torch.zeros(1, dtype=torch.int32, device=dev)
    bound.fill_(step - 1)
    plain.fill_(step)
    ops.opt_step_begin(bound, ops.make_hyper("adam", 0.01), consts)
    assert int(bound) == step and int(consts[0]) == step
    try:
        _three_kernels(torch, ops, "adam", a, bound, 8)
    finally:
        ops.opt_step_unbind(bound)
    _three_kernels(torch, ops, "adam", b, plain, 8)
    _equal_bits(torch, a, b)
    # the two floats themselves: torch's double-precision expressions over the hyper's fp32 values, rounded once
    lr, b1, b2 = (float(torch.tensor(x, dtype=torch.float32)) for x in (0.01, 0.9, 0.999))
    want = torch.tensor([lr / (1.0 - b1 ** step), 1.0 / (1.0 - b2 ** step) ** 0.5], dtype=torch.float64)
    got = consts[1:3].view(torch.float32).cpu().double()
    assert float(((got - want).abs() / want).max()) < 2e-7


@pytest.mark.parametrize("kind", ["rmsprop", "adagrad", "sgd"])
def test_other_optimizers_unchanged(env, kind):
    torch, L, ops = env
    dev = torch.device("cuda:0")
    a, b = _dense_case(torch, ops, kind, 8, 6), _dense_case(torch, ops, kind, 8, 6)
    bound, consts = ops.step_counter(dev)
    plain = torch.ones(1, dtype=torch.int32, device=dev)
    ops.opt_step_begin(bound, ops.make_hyper(kind, 0.01), consts)
    try:
        _three_kernels(torch, ops, kind, a, bound, 8)
    finally:
        ops.opt_step_unbind(bound)
    _three_kernels(torch, ops, kind, b, plain, 8)
    _equal_bits(torch, a, b)


def test_stale_constants_are_not_used(env):
    """Somebody moves the counter behind the library's back (a plain tensor write): the kernels see that the buffer names
    another step and compute the constants themselves."""
    torch, L, ops = env
    dev = torch.device("cuda:0")
    a, b = _dense_case(torch, ops, "adam", 8, 7), _dense_case(torch, ops, "adam", 8, 7)
    bound, consts = ops.step_counter(dev)
    ops.opt_step_begin(bound, ops.make_hyper("adam", 0.01), consts)   # constants of step 1 ...
    bound.fill_(40)                                                   # ... and the counter at 40
    try:
        _three_kernels(torch, ops, "adam", a, bound, 8)
    finally:
        ops.opt_step_unbind(bound)
    _three_kernels(torch, ops, "adam", b, torch.full((1,), 40, dtype=torch.int32, device=dev), 8)
    _equal_bits(torch, a, b)


def test_captured_begin_and_launch_replay(env):
    """A captured [bump + constants, dense launch] replayed three times against three eager unbound steps: the constants are
    read when the graph runs, not when it was captured."""
    torch, L, ops = env
    dev = torch.device("cuda:0")
    a, b = _dense_case(torch, ops, "adam", 8, 8), _dense_case(torch, ops, "adam", 8, 8)
    bound, consts = ops.step_counter(dev)
    h = ops.make_hyper("adam", 0.01, step=0, step_dev=bound, max_blocks=300)
    ga = a["g"].clone()
    marks, warm = a["marks"].clone(), a["warm"].clone()
    ent = [(a["p"], a["g"], a["m"], a["v"], None, None, marks, None, warm)]
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                ops.opt_step_begin(bound, h, consts)
                ops.opt_step_dense(ent, h)
        torch.cuda.synchronize()
        assert int(bound) == 0                                        # (capture ran nothing)
        for _ in range(3):
            marks.copy_(a["marks"])
            a["g"].copy_(ga)
            graph.replay()
        torch.cuda.synchronize()
    finally:
        ops.opt_step_unbind(bound)
    assert int(bound) == 3 and int(consts[0]) == 3
    plain = torch.zeros(1, dtype=torch.int32, device=dev)
    marks_b, warm_b = b["marks"].clone(), b["warm"].clone()
    for _ in range(3):
        ops.counter_update(plain, 1)
        marks_b.copy_(b["marks"])
        b["g"].copy_(ga)
        ops.opt_step_dense([(b["p"], b["g"], b["m"], b["v"], None, None, marks_b, None, warm_b)],
                           ops.make_hyper("adam", 0.01, step=0, step_dev=plain, max_blocks=300))
    for k in ("p", "m", "v", "g"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert torch.equal(warm, warm_b) and int(marks.max()) == 0
