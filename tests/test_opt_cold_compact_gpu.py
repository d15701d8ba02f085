"""The wave-compacted loop of the marked streaming table update over a warm map (mml_opt_hyper.cold_loop = 0, csrc/optim.hip):
a lane reads a dword of marks and a dword of warm bytes, the wave lists its live rows and shares their chunks out.

Every case is ONE launch over seven small tables (1 .. 1 025 rows: smaller than a span, one row more or less than a span
boundary) and one table of (1 << 24) // E + 37 rows (the streaming launch exists from 2^24 parameters up), two steps in a
row, compared bit for bit with the same launch without a map from the same state and the same gradient bits: p, m, v, the
gradient, the 64-bit totals and the marks are equal, the warm map is exactly (old warm OR marked).  The maps are views into
larger buffers with non-zero bytes directly before and after them and the tensors carry two canary rows behind their last
row: a kernel that took a byte at an index >= rows for a live row would update a canary row.

Which cases run the compacted loop: form 4 with either cap, and form 3 with max_blocks = 300.  Form 3 with max_blocks = 0 is
launched as the plain loop form (mml_opt_step_dense picks the marked form 3 only under a workgroup cap), whose remainder loop
reads the maps byte by byte: those cases, the odd-address cases and the cold_loop = 1 cases check the other loops against the
same reference.  The comparison is bitwise and all loops give the same bits, so no case can tell which loop ran; that the
compacted loop is the one the capped and form-4 launches take is read from the code (csrc/optim.hip: `compact`)."""
import functools

import pytest

pytestmark = pytest.mark.gpu

SMALL = (1, 3, 5, 255, 257, 1023, 1025)
# The issue's eight patterns, plus random 15 % (spans on both sides of the share of live rows from which the kernel walks a
# span row by row instead of listing its live rows) and 70 % (row-by-row walk with holes).
PATTERNS = ("none", "row0", "last", "every257", "span", "all", "rand4", "rand40", "rand15", "rand70")
CANARY = 0xA5


@pytest.fixture(scope="module")
def env():
    import torch
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, ops
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch, L, ops


def _pattern(torch, name, V, step, dev):
    """(marked, warm) of a table of V rows as bool tensors; live = marked | warm.  Whatever is live mixes marked-and-cold,
    marked-and-warm and unmarked-and-warm rows by the row number, so that a map dword holds all four combinations."""
    r = torch.arange(V, device=dev)
    kind = (r + step) % 3                                     # 0: marked, cold   1: marked, warm   2: warm only
    if name == "none":
        live = torch.zeros(V, dtype=torch.bool, device=dev)
    elif name == "row0":
        live = r == 0
    elif name == "last":
        live = r == V - 1
    elif name == "every257":                                  # 257 = 1 mod 4 and mod 256: every lane, every byte position
        live = r % 257 == 0
        kind = (r // 257 + step) % 3
    elif name == "span":                                      # rows 1 024 .. 2 047 live, their neighbours cold
        live = (r >= 1024) & (r < 2048)
    elif name == "all":
        live = torch.ones(V, dtype=torch.bool, device=dev)
        kind = torch.where(r % 5 == 0, (r // 5 + step) % 2, torch.full_like(r, 2))  # a fifth of the rows marked
    else:
        g = torch.Generator(device=dev).manual_seed(1000 * step + V % 997)
        u = torch.rand(V, generator=g, device=dev)
        # warm and marked independently: 4 % / 40 % / 15 % / 70 % live
        q, m = {"rand4": (0.03, 0.0103), "rand40": (0.36, 0.0625), "rand15": (0.12, 0.035), "rand70": (0.66, 0.12)}[name]
        warm = u < q
        marked = (u * 7919.0) % 1.0 < m
        return marked, warm
    return live & (kind <= 1), live & (kind >= 1)


@functools.lru_cache(maxsize=1)
def _masters(E):
    """Per width, built once and never written: the tables' start values, moments for the warm rows, and the buffers."""
    import torch
    dev = torch.device("cuda:0")
    vocab = list(SMALL) + [(1 << 24) // E + 37]
    g = torch.Generator(device=dev).manual_seed(17 + E)
    p0 = [torch.randn(v + 2, E, generator=g, device=dev) for v in vocab]
    m0 = [torch.randn(v + 2, E, generator=g, device=dev) * 0.1 + 0.01 for v in vocab]
    v0 = [torch.rand(v + 2, E, generator=g, device=dev) + 0.01 for v in vocab]
    return vocab, p0, m0, v0


def _map_views(torch, vocab, odd, dev):
    """One byte buffer full of canaries and a zeroed view of V bytes per table; the views start at multiples of 32 (as
    ops.marks_bytes lays the marks out), or one byte behind one (odd), with at least one canary byte between two views."""
    offs, at = [], 32
    for v in vocab:
        offs.append(at + (1 if odd else 0))
        at = (offs[-1] + v + 1 + 31) // 32 * 32
    buf = torch.full((at + 32,), CANARY, dtype=torch.uint8, device=dev)
    views = [buf[o:o + v] for o, v in zip(offs, vocab)]
    for w in views:
        w.zero_()
    inside = torch.zeros(at + 32, dtype=torch.bool, device=dev)
    for o, v in zip(offs, vocab):
        inside[o:o + v] = True
    return buf, views, ~inside


def _run(env, E, form, cap, name, odd=False, cold_loop=0):
    torch, L, ops = env
    dev = torch.device("cuda:0")
    vocab, p0, m0, v0 = _masters(E)
    F = len(vocab)
    std_base = [0]
    for v in vocab:
        std_base.append(std_base[-1] + (v + 31) // 32 * 32)
    marks_std = torch.zeros(ops.marks_bytes(vocab), dtype=torch.uint8, device=dev)
    mbuf, marks, m_out = _map_views(torch, vocab, odd, dev)
    wbuf, warm, w_out = _map_views(torch, vocab, odd, dev)
    mbuf_r, marks_r, _ = _map_views(torch, vocab, odd, dev)
    for f, v in enumerate(vocab):
        assert marks[f].data_ptr() % 4 == (1 if odd else 0) and warm[f].data_ptr() % 4 == (1 if odd else 0)
        assert int(mbuf[marks[f].data_ptr() - mbuf.data_ptr() - 1]) == CANARY          # directly before ...
        assert int(mbuf[marks[f].data_ptr() - mbuf.data_ptr() + v]) == CANARY          # ... and directly after
    # state: the warm rows carry moments, the cold ones zeros (what the map promises); two canary rows behind each tensor
    warm0 = [_pattern(torch, name, v, 0, dev)[1] for v in vocab]
    full = {"p": [x.clone() for x in p0], "m": [], "v": [], "g": [], "acc": []}
    for f, v in enumerate(vocab):
        keep = torch.cat([warm0[f], torch.ones(2, dtype=torch.bool, device=dev)]).view(-1, 1)
        full["m"].append(torch.where(keep, m0[f], torch.zeros_like(m0[f])))  # (+0.0: a product with False gives -0.0)
        full["v"].append(torch.where(keep, v0[f], torch.zeros_like(v0[f])))
        full["g"].append(torch.cat([torch.zeros(v, E, device=dev), torch.full((2, E), 3.0, device=dev)]))
        full["acc"].append(torch.cat([torch.zeros(v, E, dtype=torch.int64, device=dev),
                                      torch.full((2, E), 12345, dtype=torch.int64, device=dev)]))
        warm[f].copy_(warm0[f].to(torch.uint8))
    ref = {k: [x.clone() for x in xs] for k, xs in full.items()}
    canaries = {k: [x[v:].clone() for x, v in zip(xs, vocab)] for k, xs in full.items()}
    view = lambda d, k: [x[:v] for x, v in zip(d[k], vocab)]  # noqa: E731
    slot = ops.amax_slots(1, dev)[0]
    for step in (1, 2):
        want = [_pattern(torch, name, v, step, dev)[0].nonzero().view(-1) for v in vocab]
        B = max(int(w.numel()) for w in want)
        shift = ops.scatter_det_shift(max(B, 1))
        if B:                                                                    # (a table with no row to mark lends row 0)
            X = torch.stack([torch.cat([w, (w[:1] if w.numel() else w.new_zeros(1)).repeat(B - w.numel())])
                             for w in want], 1).to(torch.float32).contiguous()
            assert torch.equal(X[:want[F - 1].numel(), F - 1].long(), want[F - 1])  # (row ids below 2^24 are exact floats)
            gd = torch.Generator(device=dev).manual_seed(step)
            d = torch.randn(B, F * E, generator=gd, device=dev)
            if form == 4:
                slot.zero_()
                ops.amax_batch([(d, slot)])
                ops.scatter_bwd_det(view(full, "g"), X, list(range(F)), d, view(full, "acc"), marks_std, amax_slot=slot,
                                    clear_marks=False, amax_supplied=True, defer_totals=True)
                assert int(full["acc"][F - 1][:vocab[F - 1]].abs().max()) > 0
            else:
                ops.scatter_bwd(view(full, "g"), X, list(range(F)), d, marks=marks_std)
        marked, old_warm = [], []
        for f, v in enumerate(vocab):                                            # the scatter's marks, moved behind canaries
            marks[f].copy_(marks_std[std_base[f]:std_base[f] + v])
            marks_r[f].copy_(marks[f])
            marked.append(marks[f] != 0)
            old_warm.append(warm[f] != 0)
            assert int(marked[f].sum()) >= int(want[f].numel())
            ref["g"][f].copy_(full["g"][f])                                      # the same gradient bits in both runs
            ref["acc"][f].copy_(full["acc"][f])
        marks_std.zero_()
        hyper = ops.make_hyper("adam", 0.01, step=step, zero_grad=True, max_blocks=cap, cold_loop=cold_loop)
        det = (lambda d_, f: (d_["acc"][f][:vocab[f]], slot, shift)) if form == 4 else (lambda d_, f: None)
        ent = lambda d_, mk, wm: [(d_["p"][f][:v], d_["g"][f][:v], d_["m"][f][:v], d_["v"][f][:v], None, None, mk[f],  # noqa: E731
                                   det(d_, f), wm[f] if wm else None) for f, v in enumerate(vocab)]
        ops.opt_step_dense(ent(full, marks, warm), hyper)
        ops.opt_step_dense(ent(ref, marks_r, None), hyper)
        for f, v in enumerate(vocab):
            for k in ("p", "m", "v", "g"):
                assert torch.equal(full[k][f][:v].view(torch.int32), ref[k][f][:v].view(torch.int32)), (k, f, step)
            assert torch.equal(full["acc"][f][:v], ref["acc"][f][:v]), (f, step)
            assert torch.equal(marks[f], marks_r[f]) and int(marks[f].max()) == 0, (f, step)
            assert torch.equal(warm[f] != 0, old_warm[f] | marked[f]), (f, step)
            assert int(warm[f].max()) <= 1
            assert float(full["g"][f][:v].abs().max()) == 0.0 and int(full["acc"][f][:v].abs().max()) == 0
            for k in full:                                                       # nothing behind the last row moved
                assert torch.equal(full[k][f][v:], canaries[k][f]), (k, f, step)
        for buf, out in ((mbuf, m_out), (wbuf, w_out)):                          # every byte outside the views
            assert bool((buf[out] == CANARY).all()), step
    if name != "none":
        assert not torch.equal(full["p"][F - 1], p0[F - 1])                      # (the steps did move something)


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("cap", [0, 300])
@pytest.mark.parametrize("form", [3, 4])
@pytest.mark.parametrize("E", [4, 8, 16])
def test_compacted_loop_is_exact(env, E, form, cap, name):
    _run(env, E, form, cap, name)


@pytest.mark.parametrize("name", ["every257", "rand40"])
@pytest.mark.parametrize("form", [3, 4])
def test_unaligned_maps_take_the_byte_loop(env, form, name):
    """Map views that start at an odd address: no aligned dword holds a lane's four rows, the workgroup takes the loop
    before the compacted one -- the same bits, the same canaries."""
    _run(env, 8, form, 300, name, odd=True)


@pytest.mark.parametrize("name", ["span", "rand4"])
def test_switch_restores_the_byte_loop(env, name):
    """mml_opt_hyper.cold_loop = 1 (MMLREC_OPT_COLD_COMPACT=0) on aligned maps: the same bits."""
    _run(env, 8, 4, 300, name, cold_loop=1)
