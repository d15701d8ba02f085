"""The PCGrad kernels (csrc/pcgrad.hip: mml_pcgrad_gram / _weights / _combine / _stash) against numpy.

Shapes: T in {2, 3, 4}; flat segments of 1, 3, 255, 256, 257, 65 541 and 3 * 2^20 + 1 elements, 16-byte aligned and
misaligned by one element; table segments V in {2, 100, 5000} x E in {4, 8, 16} with no row marked, every row marked and
every seventh; one segment with a NULL bank; `out` aliasing bank[0].  More than one launch's worth of segments in one call.

Criteria: gram within n 2^-53 sum |a||b| of the exact Gram (the worst case of ANY double summation of n exact products:
derived, not measured) and bit-equal on two launches; rows whose mark is 0 are neither read (NaN there changes nothing) nor
written; weights against the float64 restatement of tests/test_pcgrad_cpu.py (equal flags, each weight within 2^-23
relative of the double value rounded to fp32); combine bit-equal to the stated fma order evaluated in numpy."""
import itertools

import numpy as np
import pytest
import torch

from test_pcgrad_cpu import weights64

pytestmark = pytest.mark.gpu

FLAT = [1, 3, 255, 256, 257, 65541, 3 * (1 << 20) + 1]
TABLES = [(V, E) for V in (2, 100, 5000) for E in (4, 8, 16)]


def fma32(w, b, acc):
    """fl32(w * b + acc) for float32 arrays, exactly: the product of two fp32 numbers is exact in double; the sum is
    rounded to ODD in double (TwoSum gives the error's sign), after which the rounding to fp32 is the correct one."""
    p = w.astype(np.float64) * b.astype(np.float64)
    a = acc.astype(np.float64)
    s = p + a
    bb = s - p
    e = (p - (s - bb)) + (a - bb)
    bits = s.view(np.int64).copy()
    fix = (e != 0) & ((bits & 1) == 0) & np.isfinite(s)
    up = (e > 0) == (s > 0)  # away from zero in the bit pattern's order
    bits[fix & up] += 1
    bits[fix & ~up] -= 1
    return bits.view(np.float64).astype(np.float32)


def test_fma32_is_a_fused_multiply_add():
    import fractions
    rng = np.random.default_rng(0)
    w, b, a = (rng.standard_normal(4096).astype(np.float32) for _ in range(3))
    got = fma32(w, b, a)
    for i in range(0, 4096, 97):
        x = fractions.Fraction(float(w[i])) * fractions.Fraction(float(b[i])) + fractions.Fraction(float(a[i]))
        lo = np.float32(float(x))  # (Fraction -> float rounds correctly to double; then double -> fp32 may double-round)
        cands = {lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))}
        best = min(cands, key=lambda c: abs(fractions.Fraction(float(c)) - x))
        assert got[i] == best, i


def build_segments(T, seed):
    """[(dict for ops, numpy banks [T] or None, marks numpy or None)], data on cuda:0."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    dev = torch.device("cuda:0")
    segs = []

    def banks(shape, null=None, shift=0):
        out = []
        for t in range(T):
            if t == null:
                out.append(None)
                continue
            n = int(np.prod(shape))
            buf = torch.randn(n + 8, generator=gen, device=dev)
            out.append(buf[shift:shift + n].view(shape))
        return out

    for n in FLAT:
        for shift in (0, 1):
            segs.append(dict(banks=banks((n,), shift=shift), out=torch.full((n + 8,), 7.0, device=dev)[shift:shift + n]))
    for V, E in TABLES:
        for kind in ("none", "all", "seventh"):
            marks = torch.zeros(V, dtype=torch.uint8, device=dev)
            if kind == "all":
                marks[:] = 1
            elif kind == "seventh":
                marks[::7] = 1
            segs.append(dict(banks=banks((V, E)), out=torch.full((V, E), 7.0, device=dev), marks=marks))
    segs.append(dict(banks=banks((300, 12)), out=torch.full((300, 12), 7.0, device=dev)))   # unmarked table, E % 4 == 0
    segs.append(dict(banks=banks((77, 5), null=1), out=torch.full((77, 5), 7.0, device=dev)))  # a NULL bank, odd width
    alias = dict(banks=banks((513, 8)))
    alias["out"] = alias["banks"][0]  # out aliases bank[0]
    segs.append(alias)
    return segs


def host(seg):
    return [None if b is None else b.cpu().numpy().astype(np.float32) for b in seg["banks"]], \
        (None if seg.get("marks") is None else seg["marks"].cpu().numpy().astype(bool))


@pytest.fixture(scope="module", params=[2, 3, 4])
def setup(request):
    T = request.param
    segs = build_segments(T, 100 + T)
    ref = [host(sg) for sg in segs]
    # exact Gram (long double accumulation of exact products) and the bound's sum |a||b|
    G, S, n = np.zeros((T, T), np.longdouble), np.zeros((T, T), np.longdouble), 0
    for banks, marks in ref:
        rows = slice(None) if marks is None else marks
        live = [None if b is None else b.reshape(b.shape[0], -1)[rows].astype(np.longdouble) if b.ndim == 2
                else b.astype(np.longdouble) for b in banks]
        n += next(x.size for x in live if x is not None)
        for a in range(T):
            for b in range(a, T):
                if live[a] is not None and live[b] is not None:
                    G[a, b] += (live[a] * live[b]).sum()
                    S[a, b] += (np.abs(live[a]) * np.abs(live[b])).sum()
                    G[b, a], S[b, a] = G[a, b], S[a, b]
    return T, segs, ref, G, S, n


def test_gram_bound_and_repeatability(setup):
    from mmlrec_amd import ops
    T, segs, ref, G, S, n = setup
    assert len(segs) > 24  # more than one launch of segments
    g1 = ops.pcgrad_gram(segs, T).cpu().numpy()
    g2 = ops.pcgrad_gram(segs, T).cpu().numpy()
    assert g1.tobytes() == g2.tobytes()
    assert (g1 == g1.T).all()
    err = np.abs(g1.astype(np.longdouble) - G)
    bound = n * 2.0 ** -53 * S
    print(f"[T={T}] n={n} worst |gram - exact| / bound = {float((err / bound).max()):.3g}")
    assert (err <= bound).all(), (err / bound)


def test_unmarked_rows_are_not_read_and_not_written(setup):
    from mmlrec_amd import ops
    T, segs, ref, G, S, n = setup
    before = ops.pcgrad_gram(segs, T).cpu().numpy()
    w = torch.tensor(np.linspace(0.5, 1.5, 2 * T), dtype=torch.float32, device="cuda")
    saved = []
    for sg in segs:
        if sg.get("marks") is None:
            continue
        off = ~sg["marks"].bool()
        saved.append((sg, [b[off].clone() for b in sg["banks"]]))
        for b in sg["banks"]:
            b[off] = float("nan")
        sg["out"].fill_(7.0)
    try:
        after = ops.pcgrad_gram(segs, T).cpu().numpy()
        assert before.tobytes() == after.tobytes()
        marked = [sg for sg in segs if sg.get("marks") is not None]
        ops.pcgrad_combine(marked, T, w)
        for sg in marked:
            off = ~sg["marks"].bool()
            out = sg["out"]
            assert bool((out[off] == 7.0).all())                       # untouched
            assert bool(torch.isfinite(out[~off]).all()) and (int((~off).sum()) == 0 or bool((out[~off] != 7.0).any()))
    finally:
        for sg, rows in saved:
            off = ~sg["marks"].bool()
            for b, r in zip(sg["banks"], rows):
                b[off] = r


def test_combine_is_the_stated_fma_chain(setup):
    from mmlrec_amd import ops
    T, segs, ref, G, S, n = setup
    rng = np.random.default_rng(5 + T)
    w = rng.standard_normal(2 * T).astype(np.float32)
    for sg in segs:
        if sg["out"] is not sg["banks"][0]:
            sg["out"].fill_(7.0)
    ops.pcgrad_combine(segs, T, torch.from_numpy(w).cuda())
    for sg, (banks, marks) in zip(segs, ref):
        wk = w[:T] if all(b is not None for b in banks) else w[T:]
        shape = next(b for b in banks if b is not None).shape
        acc = np.zeros(shape, np.float32).ravel()
        for k in range(T):
            if banks[k] is not None:
                acc = fma32(np.full(acc.shape, wk[k], np.float32), banks[k].ravel(), acc)
        want = acc.reshape(shape)
        if marks is not None:
            want = np.where(marks[:, None], want, np.float32(7.0))
        got = sg["out"].cpu().numpy()
        assert got.tobytes() == want.astype(np.float32).tobytes(), (shape, marks is not None)
    # the aliasing segment's bank[0] now holds the result: restore it for the tests that follow
    alias = next(i for i, sg in enumerate(segs) if sg["out"] is sg["banks"][0])
    segs[alias]["banks"][0].copy_(torch.from_numpy(ref[alias][0][0]).cuda())


def test_stash_moves_marked_rows_and_clears_them(setup):
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, ops
    T, segs, ref, G, S, n = setup
    lib = L.load()
    for clear in (0, 1):
        items, srcs = [], []
        for sg in segs[:3] + [sg for sg in segs if sg.get("marks") is not None][:9]:
            src = sg["banks"][0].clone()
            dst = torch.full_like(src, 7.0)
            items.append(dict(banks=[src], out=dst, marks=sg.get("marks")))
            srcs.append(src.clone())
        arr = ops.make_pcgrad_segs(items, 1, need_out=True)
        L.check(lib.mml_pcgrad_stash(arr, len(items), clear, torch.cuda.current_stream().cuda_stream), "mml_pcgrad_stash")
        for it, src0 in zip(items, srcs):
            m = it.get("marks")
            on = torch.ones(src0.shape[0], dtype=torch.bool, device="cuda") if (m is None or src0.dim() == 1) else m.bool()
            if src0.dim() == 1:
                assert torch.equal(it["out"], src0)
                assert torch.equal(it["banks"][0], torch.zeros_like(src0) if clear else src0)
                continue
            assert torch.equal(it["out"][on], src0[on]) and bool((it["out"][~on] == 7.0).all())
            assert torch.equal(it["banks"][0][~on], src0[~on])
            assert torch.equal(it["banks"][0][on], torch.zeros_like(src0[on]) if clear else src0[on])


def run_weights(G, orders):
    from mmlrec_amd import ops
    T = G.shape[0]
    w, fired = ops.pcgrad_weights(torch.from_numpy(np.ascontiguousarray(G, np.float64)).cuda(),
                                  torch.tensor(orders, dtype=torch.int32, device="cuda"))
    c, fired64 = weights64(np.asarray(G, np.float64), orders)
    assert (fired.cpu().numpy() == fired64).all(), (orders, fired.cpu().numpy(), fired64)
    want = np.concatenate([c.sum(0) / T, c.sum(0)])
    got = w.cpu().numpy().astype(np.float64)
    w32 = want.astype(np.float32).astype(np.float64)
    assert (np.abs(got - w32) <= 2.0 ** -23 * np.abs(want)).all(), (got, want)
    return fired64, want


def test_weights_hand_built_grams():
    # all dots positive: nothing fires, mean weights 1 / T, sum weights 1
    V = np.array([[1.0, 0.2, 0.1], [0.3, 1.0, 0.2], [0.2, 0.1, 1.0]])
    fired, want = run_weights(V @ V.T, [[0, 1, 2], [2, 1, 0], [1, 0, 2]])
    assert fired.sum() == 0 and np.allclose(want[:3], 1 / 3) and np.allclose(want[3:], 1.0)
    # an orthogonal pair: d == 0 is no conflict
    fired, want = run_weights(np.diag([2.0, 5.0]), [[1, 0], [0, 1]])
    assert fired.sum() == 0 and np.allclose(want, [0.5, 0.5, 1.0, 1.0])
    # a zero gradient: G[j][j] == 0 meets d == 0 only
    fired, want = run_weights(np.array([[0.0, 0.0], [0.0, 3.0]]), [[1, 0], [1, 0]])
    assert fired.sum() == 0
    # T = 2 in conflict: both project
    V = np.array([[1.0, 0.0], [-0.6, 0.8]])
    fired, want = run_weights(V @ V.T, [[0, 1], [1, 0]])
    assert fired.tolist() == [[0, 1], [1, 0]]
    # T = 3, a chain of conflicts, under each of the 6 orders (the same order for every i, and a mix of all six)
    V = np.array([[1.0, 0.3, -0.2], [-0.8, 1.0, 0.1], [0.3, -0.9, 1.0]])
    G = V @ V.T
    assert G[0, 1] < 0 and G[1, 2] < 0 and G[0, 2] < 0
    perms = [list(p) for p in itertools.permutations(range(3))]
    seen = set()
    for p in perms:
        fired, want = run_weights(G, [p, p, p])
        assert fired.sum() >= 3
        seen.add(tuple(np.round(want, 12)))
    assert len(seen) > 1  # the order matters
    for k in range(6):
        run_weights(G, [perms[k], perms[(k + 1) % 6], perms[(k + 3) % 6]])
    # T = 4 with a Gram taken from random vectors
    rng = np.random.default_rng(3)
    V = rng.standard_normal((4, 6))
    run_weights(V @ V.T, [[3, 1, 0, 2], [0, 2, 3, 1], [1, 0, 2, 3], [2, 3, 1, 0]])


def test_every_bad_argument_returns_err_arg():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    a, b, out = (torch.zeros(16, 4, device="cuda") for _ in range(3))
    gram = torch.zeros(4, 4, dtype=torch.float64, device="cuda")
    w = torch.zeros(8, device="cuda")
    order = torch.zeros(16, dtype=torch.int32, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")

    def seg(ld=4, banks=(a, b), o=out):
        arr = (L.PcgradSeg * 1)()
        for k, t in enumerate(banks):
            arr[0].bank[k] = t.data_ptr() if t is not None else None
        arr[0].out = o.data_ptr() if o is not None else None
        arr[0].rows, arr[0].cols, arr[0].ld = 16, 4, ld
        return arr

    ok = seg()
    need = lib.mml_pcgrad_workspace_bytes(ok, 1, 2)
    assert 0 < need <= ws.numel()
    assert lib.mml_pcgrad_gram(ok, 1, 2, gram.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
    assert lib.mml_pcgrad_combine(ok, 1, 2, w.data_ptr(), st) == 0
    for T in (0, 9):
        assert lib.mml_pcgrad_gram(ok, 1, T, gram.data_ptr(), ws.data_ptr(), ws.numel(), st) == -1
        assert lib.mml_pcgrad_combine(ok, 1, T, w.data_ptr(), st) == -1
        assert lib.mml_pcgrad_weights(gram.data_ptr(), order.data_ptr(), T, w.data_ptr(), None, st) == -1
    assert lib.mml_pcgrad_gram(ok, 0, 2, gram.data_ptr(), ws.data_ptr(), ws.numel(), st) == -1          # n < 1
    assert lib.mml_pcgrad_combine(ok, 0, 2, w.data_ptr(), st) == -1
    assert lib.mml_pcgrad_gram(seg(ld=3), 1, 2, gram.data_ptr(), ws.data_ptr(), ws.numel(), st) == -1   # ld < cols
    assert lib.mml_pcgrad_combine(seg(ld=3), 1, 2, w.data_ptr(), st) == -1
    none = seg(banks=(None, None))
    assert lib.mml_pcgrad_gram(none, 1, 2, gram.data_ptr(), ws.data_ptr(), ws.numel(), st) == -1        # every bank NULL
    assert lib.mml_pcgrad_combine(none, 1, 2, w.data_ptr(), st) == -1
    assert lib.mml_pcgrad_combine(seg(o=None), 1, 2, w.data_ptr(), st) == -1                            # null out
    assert lib.mml_pcgrad_gram(ok, 1, 2, gram.data_ptr(), ws.data_ptr(), need - 1, st) == -1            # short workspace
    assert lib.mml_pcgrad_gram(ok, 1, 2, gram.data_ptr(), None, need, st) == -1
    assert b"workspace" in lib.mml_last_error()
    torch.cuda.synchronize()
