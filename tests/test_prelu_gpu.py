"""The PReLU kernels alone (include/mmlrec.h: mml_prelu_batch_fwd / _bwd, csrc/prelu.hip) against numpy written here.

y and dz are ONE IEEE multiply per element, so they are compared bit for bit with the float32 restatement
np.where(z > 0, z, a * z) / np.where(z > 0, dy, a * dy).  The slope gradient da = sum_{z <= 0} dy * z is a sum whose order
the kernel fixes but does not document, so it is held to what holds for ANY fp32 order: the project's 1e-4 max-norm
criterion where nothing cancels (dy > 0 everywhere: every term has the sign of z <= 0), and the worst-case bound
|got - ref64| <= (n + 1) 2^-24 sum |dy z| where terms cancel (n elements: n - 1 additions and one product rounding per
term; the kernel's double-precision final sum and fp32 partials only do better).  z holds subnormals, and a product in the
subnormal range rounds to the fp32 subnormal spacing 2^-149 absolutely, not to 2^-24 of itself: the bound carries that
underflow term, n 2^-149 -- 1e-45 per element, which matters only where nothing but such a term enters the sum (the
1 x 1 items)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-4  # RTOL of tests/test_models_gpu.py
ROWS, COLS = (1, 63, 4173), (1, 6, 16, 250)
SLOPES = (0.25, 0.0, -0.5, 1.0)
PAD = 777.0  # what the padding columns hold before a launch
U = 2.0 ** -24
ETA = 2.0 ** -149  # spacing of fp32 subnormals


@pytest.fixture(scope="module")
def env():
    import torch
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, ops
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch, L, ops


def shapes():
    """(rows, cols, ld, base offset in elements): ld = cols rounded up to 16 (16-byte path, ragged tails, padding), plus one
    unpadded item at an odd offset (the single-element path)."""
    out = [(r, c, (c + 15) // 16 * 16, 0) for r in ROWS for c in COLS]
    out.append((63, 6, 6, 1))
    return out


class Item:
    """Host and device buffers of one problem.  z holds +0.0, -0.0 and subnormals of both signs among normal draws."""

    def __init__(self, torch, shape, slope, seed, dy_positive=False):
        self.rows, self.cols, self.ld, self.off = shape
        rng = np.random.default_rng(seed)
        n = self.rows * self.cols
        z = rng.standard_normal(n).astype(np.float32)
        special = np.array([0.0, -0.0, 1e-40, -1e-40], np.float32)
        pos = rng.permutation(n)[:min(n, 4)]
        z[pos] = special[(seed + np.arange(len(pos))) % 4]
        dy = rng.standard_normal(n).astype(np.float32)
        if dy_positive:
            dy = np.abs(dy) + np.float32(0.01)
        self.z, self.dy = z.reshape(self.rows, self.cols), dy.reshape(self.rows, self.cols)
        self.a = np.float32(slope)
        dev = torch.device("cuda:0")
        self.torch = torch
        self.zb, self.dyb = self._buf(self.z), self._buf(self.dy)
        self.yb, self.dzb = self._buf(None), self._buf(None)
        self.alpha = torch.tensor([slope], dtype=torch.float32, device=dev)
        self.dalpha = torch.full((1,), 12345.0, dtype=torch.float32, device=dev)

    def _buf(self, host):
        torch = self.torch
        flat = torch.full((self.off + self.rows * self.ld,), PAD, dtype=torch.float32, device="cuda:0")
        v = flat[self.off:].view(self.rows, self.ld)[:, :self.cols]
        if host is not None:
            v.copy_(torch.from_numpy(host))
        return flat

    def view(self, flat):
        return flat[self.off:].view(self.rows, self.ld)[:, :self.cols]

    def padding_untouched(self, flat):
        h = flat.cpu().numpy()
        body = h[self.off:].reshape(self.rows, self.ld)
        return np.all(h[:self.off] == PAD) and np.all(body[:, self.cols:] == PAD)

    # float32 restatements: one multiply, rounded once
    def y_ref(self):
        return np.where(self.z > 0, self.z, self.a * self.z)

    def dz_ref(self):
        return np.where(self.z > 0, self.dy, self.a * self.dy)

    def da_terms(self):
        return np.where(self.z <= 0, self.dy.astype(np.float64) * self.z.astype(np.float64), 0.0)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def slot_bits(torch, slot):
    return int(slot.view(torch.int32).max())


def amax_bits(x):
    return int(np.abs(np.asarray(x, np.float32)).max().view(np.uint32)) if x.size else 0


def run_fwd(env, items, slots=None):
    torch, L, ops = env
    ops.prelu_fwd([dict(z=it.view(it.zb), y=it.view(it.yb), alpha=it.alpha, amax=None if slots is None else slots[i])
                   for i, it in enumerate(items)])
    torch.cuda.synchronize()


def run_bwd(env, items, slots=None, dz=None, acc_dz=False, dalpha=None, acc_dalpha=False):
    torch, L, ops = env
    ops.prelu_bwd([dict(dy=it.view(it.dyb), z=it.view(it.zb), dz=it.view(it.dzb if dz is None else dz[i]), alpha=it.alpha,
                        dalpha=it.dalpha if dalpha is None else dalpha[i], acc_dz=acc_dz, acc_dalpha=acc_dalpha,
                        amax=None if slots is None else slots[i]) for i, it in enumerate(items)])
    torch.cuda.synchronize()


def check_da(got, items):
    terms = np.concatenate([it.da_terms().ravel() for it in items])
    ref, n = float(terms.sum()), terms.size
    bound = (n + 1) * U * float(np.abs(terms).sum()) + n * ETA
    print(f"  da got {got:.9g} ref64 {ref:.9g} |diff| {abs(got - ref):.3g} bound {bound:.3g} (n = {n})")
    assert abs(got - ref) <= bound, (got, ref, bound)


def launch_sets(ops):
    """Launches of 1, 5 and the cap's number of mixed-shape items; every shape and every slope occurs."""
    sh, cap = shapes(), ops.prelu_max_batch()
    sets = [[(s, SLOPES[(i + j) % 4])] for i, s in enumerate(sh) for j in range(1 if s[0] > 63 else 4)]
    sets.append([(sh[(3 * k + 1) % len(sh)], SLOPES[k % 4]) for k in range(5)])
    sets.append([(sh[k % len(sh)], SLOPES[(k // 2) % 4]) for k in range(cap)])
    return sets


def test_cap_covers_a_grouped_launch(env):
    torch, L, ops = env
    assert ops.prelu_max_batch() >= L.MAX_GROUP


def test_forward_backward_bit_for_bit_over_the_grid(env):
    torch, L, ops = env
    sizes = set()
    for si, spec in enumerate(launch_sets(ops)):
        items = [Item(torch, s, a, 1000 * si + k) for k, (s, a) in enumerate(spec)]
        sizes.add(len(items))
        slots = ops.amax_slots(2 * len(items), "cuda:0")
        fs, bs = slots[:len(items)], slots[len(items):]
        run_fwd(env, items, fs)
        run_bwd(env, items, bs)
        first = [float(it.dalpha.item()) for it in items]
        dz1 = [it.view(it.dzb).cpu().numpy().copy() for it in items]
        for it in items:
            it.dalpha.fill_(-1.0)
        run_bwd(env, items)  # (without magnitude slots: dz does not depend on how many workgroups walk an item)
        for k, it in enumerate(items):
            y, dz = it.view(it.yb).cpu().numpy(), it.view(it.dzb).cpu().numpy()
            assert np.array_equal(bits(y), bits(it.y_ref())), (spec[k], "y")
            assert np.array_equal(bits(dz), bits(it.dz_ref())), (spec[k], "dz")
            assert np.array_equal(bits(dz1[k]), bits(dz))
            assert it.padding_untouched(it.yb) and it.padding_untouched(it.dzb), (spec[k], "padding")
            assert it.padding_untouched(it.zb) and it.padding_untouched(it.dyb)
            assert slot_bits(torch, fs[k]) == amax_bits(y), (spec[k], "amax y")
            assert slot_bits(torch, bs[k]) == amax_bits(dz), (spec[k], "amax dz")
            check_da(first[k], [it])
    assert sizes == {1, 5, ops.prelu_max_batch()}


def test_two_launches_give_identical_bits(env):
    torch, L, ops = env
    items = [Item(torch, s, SLOPES[k % 4], 50 + k) for k, s in enumerate(shapes())]
    slots = ops.amax_slots(len(items), "cuda:0")
    got = []
    for _ in range(2):
        for it in items:
            it.dalpha.fill_(3.0)
        slots.zero_()
        run_bwd(env, items, slots)
        got.append(np.array([it.dalpha.item() for it in items], np.float32))
    assert np.array_equal(bits(got[0]), bits(got[1]))


def test_accumulate_dz_and_aliasing(env):
    torch, L, ops = env
    for k, s in enumerate(shapes()):
        it = Item(torch, s, SLOPES[k % 4], 200 + k)
        rng = np.random.default_rng(k)
        pre = rng.standard_normal((it.rows, it.cols)).astype(np.float32)
        it.view(it.dzb).copy_(torch.from_numpy(pre))
        run_bwd(env, [it], acc_dz=True)
        dz = it.view(it.dzb).cpu().numpy()
        assert np.array_equal(bits(dz), bits(pre + it.dz_ref())), s  # (the product rounds before the add)
        assert it.padding_untouched(it.dzb)
        da = float(it.dalpha.item())
        # dz aliasing dy: same bits, same slope gradient
        it.dalpha.fill_(0.0)
        run_bwd(env, [it], dz=[it.dyb])
        assert np.array_equal(bits(it.view(it.dyb).cpu().numpy()), bits(it.dz_ref())), s
        assert it.padding_untouched(it.dyb)
        assert bits(np.float32(it.dalpha.item())) == bits(np.float32(da))


def test_slope_gradient_without_cancellation(env):
    torch, L, ops = env
    for k, s in enumerate(shapes()):
        it = Item(torch, s, SLOPES[k % 4], 300 + k, dy_positive=True)
        run_bwd(env, [it])
        ref = float(it.da_terms().sum())
        got = float(it.dalpha.item())
        if ref == 0.0:  # (a single element with z > 0)
            assert got == 0.0
            continue
        print(f"  {s}: da {got:.9g} ref64 {ref:.9g} rel {abs(got - ref) / abs(ref):.3g}")
        assert abs(got - ref) / abs(ref) < RTOL, (s, got, ref)


def test_shared_and_accumulated_slope_gradient(env):
    torch, L, ops = env
    sh = shapes()
    a = Item(torch, sh[11], 0.25, 401)
    b = Item(torch, sh[6], 0.25, 402)
    c = Item(torch, sh[12], -0.5, 403)  # (a third item with a slope of its own between the two)
    shared = torch.full((1,), 9.0, dtype=torch.float32, device="cuda:0")
    run_bwd(env, [a, c, b], dalpha=[shared, c.dalpha, shared])
    both = float(shared.item())
    check_da(both, [a, b])
    check_da(float(c.dalpha.item()), [c])
    again = torch.full((1,), -4.0, dtype=torch.float32, device="cuda:0")
    run_bwd(env, [a, c, b], dalpha=[again, c.dalpha, again])
    assert bits(np.float32(again.item())) == bits(np.float32(both))
    # accumulate_dalpha: old + (the sum the launch forms), one fp32 addition
    old = np.float32(1.7)
    acc = torch.full((1,), float(old), dtype=torch.float32, device="cuda:0")
    run_bwd(env, [a, c, b], dalpha=[acc, c.dalpha, acc], acc_dalpha=True)
    assert bits(np.float32(acc.item())) == bits(old + np.float32(both))


def test_argument_refusals(env):
    torch, L, ops = env
    lib = L.load()
    cap = ops.prelu_max_batch()
    it = Item(torch, (63, 6, 16, 0), 0.25, 500)
    ws = torch.empty(int(lib.mml_prelu_workspace_bytes(cap)), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream

    def fwd(n=1, **kw):
        arr = (L.PreluDesc * max(n, cap + 1))()
        for d in arr:
            d.z, d.ldz, d.y, d.ldy = it.zb.data_ptr(), it.ld, it.yb.data_ptr(), it.ld
            d.rows, d.cols, d.alpha = it.rows, it.cols, it.alpha.data_ptr()
            for k, v in kw.items():
                setattr(d, k, v)
        return lib.mml_prelu_batch_fwd(arr, n, s)

    def bwd(n=1, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel(), **kw):
        arr = (L.PreluBwdDesc * max(n, cap + 1))()
        for d in arr:
            d.dy, d.lddy, d.z, d.ldz, d.dz, d.lddz = it.dyb.data_ptr(), it.ld, it.zb.data_ptr(), it.ld, it.dzb.data_ptr(), it.ld
            d.rows, d.cols, d.alpha, d.dalpha = it.rows, it.cols, it.alpha.data_ptr(), it.dalpha.data_ptr()
            for k, v in kw.items():
                setattr(d, k, v)
        return lib.mml_prelu_batch_bwd(arr, n, ws_ptr, ws_bytes, s)

    assert fwd() == 0 and bwd() == 0
    assert fwd(cap) == 0 and bwd(cap) == 0
    for n in (0, -1, cap + 1):
        assert fwd(n) == L.ERR_ARG and bwd(n) == L.ERR_ARG, n
    assert lib.mml_prelu_batch_fwd(None, 1, s) == L.ERR_ARG and b"null" in lib.mml_last_error()
    assert lib.mml_prelu_batch_bwd(None, 1, ws.data_ptr(), ws.numel(), s) == L.ERR_ARG
    for k in ("z", "y", "alpha"):
        assert fwd(**{k: None}) == L.ERR_ARG, k
    for k in ("dy", "z", "dz", "alpha", "dalpha"):
        assert bwd(**{k: None}) == L.ERR_ARG, k
    assert fwd(rows=-1) == L.ERR_ARG and bwd(rows=-1) == L.ERR_ARG
    assert fwd(cols=0) == L.ERR_ARG and bwd(cols=0) == L.ERR_ARG
    for k in ("ldz", "ldy"):
        assert fwd(**{k: it.cols - 1}) == L.ERR_ARG, k
    for k in ("lddy", "ldz", "lddz"):
        assert bwd(**{k: it.cols - 1}) == L.ERR_ARG, k
    assert bwd(ws_ptr=None) == L.ERR_ARG and bwd(ws_bytes=8) == L.ERR_ARG
    torch.cuda.synchronize()
    with pytest.raises(L.MMLError):
        ops.prelu_fwd([dict(z=it.view(it.zb).cpu(), y=it.view(it.yb).cpu(), alpha=it.alpha)])


def test_slope_is_read_when_the_kernel_runs(env):
    """The slope is a device pointer: a captured launch replayed after the slope changed computes with the new value."""
    torch, L, ops = env
    it = Item(torch, (63, 250, 256, 0), 0.25, 600)
    run_fwd(env, [it])
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ops.prelu_fwd([dict(z=it.view(it.zb), y=it.view(it.yb), alpha=it.alpha)])
    it.alpha.fill_(-0.5)
    it.a = np.float32(-0.5)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(it.view(it.yb).cpu().numpy()), bits(it.y_ref()))


def test_functional_prelu_against_torch_float64(env):
    torch, L, ops = env
    from mmlrec_amd import functional as F
    dev = torch.device("cuda:0")
    for k, (rows, cols) in enumerate([(63, 6), (4173, 250), (1, 1)]):
        for slope in SLOPES:
            for positive in (False, True):
                g = torch.Generator().manual_seed(700 + k)
                z = torch.randn(rows, cols, generator=g).to(dev).requires_grad_(True)
                dy = torch.randn(rows, cols, generator=g).to(dev)
                if positive:
                    dy = dy.abs() + 0.01
                a = torch.tensor([slope], device=dev, requires_grad=True)
                y = F.prelu(z, a)
                y.backward(dy)
                z64, a64 = z.detach().double().requires_grad_(True), a.detach().double().requires_grad_(True)
                y64 = torch.nn.functional.prelu(z64, a64)
                y64.backward(dy.double())
                # a product of two floats is exact in double: rounding it to float IS the fp32 multiply
                assert torch.equal(y.detach(), y64.detach().float()) and torch.equal(z.grad, z64.grad.float())
                got, ref = float(a.grad.item()), float(a64.grad.item())
                terms = torch.where(z64.detach() <= 0, dy.double() * z64.detach(), torch.zeros_like(z64.detach()))
                n = rows * cols
                assert abs(got - ref) <= (n + 1) * U * float(terms.abs().sum()) + n * ETA, (rows, cols, slope, got, ref)
                if positive and ref != 0.0:
                    assert abs(got - ref) / abs(ref) < RTOL, (rows, cols, slope, got, ref)
