"""Host-side proof of tests/opt_refs.py, without a GPU: the references the optimizer kernel tests
(tests/test_opt_parity_gpu.py) compare with are held against things they must agree with -- the oracle's float32
optimizer, a step worked out by hand, and each other -- and the conditions the GPU cases put on the reference alone
(the regulariser matters, no sign ambiguity under l1) are checked on the inputs those cases draw."""
import numpy as np
import pytest
import torch

import opt_refs as R
from oracle import mmlrec_oracle as orc


@pytest.mark.parametrize("kind", R.KINDS)
def test_dense_trajectory_matches_the_oracle_optimizer(kind):
    """oracle.DenseOptimizer (float32 numpy, defaults, no regulariser) and the float64 trajectory agree to what float32
    loses: every update within 1e-5 of the largest one."""
    rng = np.random.default_rng(3)
    p0, grads = R.draw_inputs(rng, 5003, 4)
    tr = R.dense_trajectory(kind, p0, grads, lr=0.01)
    params = {"p": p0.copy()}
    opt = orc.DenseOptimizer(kind, 0.01)
    before = p0.astype(np.float64)
    for g, (p64, _, _) in zip(grads, tr):
        old = params["p"].astype(np.float64)
        opt.step(params, {"p": g})
        upd, ref = params["p"].astype(np.float64) - old, p64 - before
        assert np.abs(upd - ref).max() <= 1e-5 * np.abs(ref).max(), kind
        before = p64


def test_adam_step_with_l1_and_l2_by_hand():
    """Three elements, p = 0 among them.  First step from zero state: m_hat = g', v_hat = g'^2, so p moves by
    lr g' / (|g'| + eps) with g' = g + l1 sign(p) + 2 l2 p.  Then step 3 from given moments, where the size of g'
    matters (a halved l2 term moves the first element by 4e-4)."""
    lr, l1, l2, eps = R.f32(0.1), R.f32(0.01), R.f32(0.02), R.f32(1e-8)
    b1, b2 = R.f32(0.9), R.f32(0.999)
    p = np.array([1.0, -0.5, 0.0])
    g = np.array([0.3, 0.2, 0.0])
    ge = [0.3 + l1 + 2 * l2 * 1.0, 0.2 - l1 + 2 * l2 * -0.5, 0.0]
    want = [1.0 - lr * ge[0] / (abs(ge[0]) + eps), -0.5 - lr * ge[1] / (abs(ge[1]) + eps), 0.0]
    (p1, m1, v1), = R.dense_trajectory("adam", p, [g], lr=0.1, l1=0.01, l2=0.02)
    assert np.abs(p1 - want).max() < 1e-12 and p1[2] == 0.0
    assert np.abs(p1 - [0.9, -0.6, 0.0]).max() < 1e-7
    assert np.abs(m1 - (1 - b1) * np.array(ge)).max() < 1e-15 and np.abs(v1 - (1 - b2) * np.array(ge) ** 2).max() < 1e-15
    # step 3 from m = 0.1, v = 0.01 on every element
    m0, v0 = 0.1, 0.01
    want3 = []
    for pe, ge_ in zip(p, ge):
        m = b1 * m0 + (1 - b1) * ge_
        v = b2 * v0 + (1 - b2) * ge_ * ge_
        want3.append(pe - lr / (1 - b1 ** 3) * m / (v ** 0.5 / (1 - b2 ** 3) ** 0.5 + eps))
    p3, _, _ = R.masked_step("adam", p, np.full(3, m0), np.full(3, v0), g, None, 3, lr=0.1, l1=0.01, l2=0.02)
    assert np.abs(p3 - want3).max() < 1e-12
    half, _, _ = R.masked_step("adam", p, np.full(3, m0), np.full(3, v0), g, None, 3, lr=0.1, l1=0.01, l2=0.01)
    assert abs(half[0] - p3[0]) > 2e-4


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", R.KINDS)
def test_masked_step_with_a_full_mask_is_the_dense_trajectory(kind, dtype):
    rng = np.random.default_rng(5)
    p0, grads = R.draw_inputs(rng, (37, 5), 3)
    kw = dict(lr=0.01, l1=1e-2, l2=1e-2, betas=(0.8, 0.95), eps=1e-6, alpha=0.9, dtype=dtype)
    tr = R.dense_trajectory(kind, p0, grads, **kw)
    p, s1, s2 = p0, None, None
    zeros = np.zeros_like(p0)
    for k, g in enumerate(grads):
        p, s1, s2 = R.masked_step(kind, p, zeros if s1 is None else s1, zeros if s2 is None else s2, g,
                                  np.ones(37, bool), k + 1, **kw)
        for a, b in zip((p, s1, s2), tr[k]):
            assert (a is None and b is None) or np.array_equal(a, b), (kind, k)


@pytest.mark.parametrize("kind", R.KINDS)
def test_masked_step_freezes_the_other_rows(kind):
    rng = np.random.default_rng(6)
    p0, (g,) = R.draw_inputs(rng, (20, 4), 1)
    s = rng.random((20, 4))
    mask = rng.random(20) < 0.5
    p, s1, s2 = R.masked_step(kind, p0, s, s, g, mask, 2, lr=0.01)
    full = R.masked_step(kind, p0, s, s, g, None, 2, lr=0.01)
    assert np.array_equal(p[~mask], p0[~mask].astype(np.float64)) and np.array_equal(p[mask], full[0][mask])
    for a, b in zip((s1, s2), full[1:]):
        if a is not None:
            assert np.array_equal(a[~mask], s[~mask]) and np.array_equal(a[mask], b[mask])


@pytest.mark.parametrize("kind", R.KINDS)
def test_zero_grad_replay_is_the_dense_trajectory_fed_zero_gradients(kind):
    """Three steps with gradients, then 30 without: the replay of (3, 33] from the state after step 3 against the
    trajectory's own end; and per-row `from` against the trajectory's intermediate states."""
    rng = np.random.default_rng(7)
    p0, grads = R.draw_inputs(rng, (11, 5), 3)
    zero = np.zeros_like(p0)
    tr = R.dense_trajectory(kind, p0, grads + [zero] * 30, lr=0.01)
    p3, m3, v3 = tr[2]
    p, m, v = R.zero_grad_replay(kind, p3, m3, v3, 3, 33, lr=0.01)
    scale = np.abs(tr[-1][0] - p3).max()
    assert np.abs(p - tr[-1][0]).max() <= 1e-12 * max(scale, 1.0)
    for a, b in ((m, tr[-1][1]), (v, tr[-1][2])):
        if b is not None:
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    if kind in ("adam", "rmsprop"):
        assert np.abs(m - m3).max() > 0          # (the replay did something)
    # row r starts from the trajectory's state after step 3 + r
    frm = 3 + np.arange(11)
    start = [np.stack([tr[f - 1][i][r] for r, f in enumerate(frm)]) if tr[0][i] is not None else None for i in range(3)]
    p, m, v = R.zero_grad_replay(kind, start[0], start[1], start[2], frm, 33, lr=0.01)
    assert np.abs(p - tr[-1][0]).max() <= 1e-12 * max(scale, 1.0)
    if m is not None:
        assert np.abs(m - tr[-1][1]).max() <= 1e-12 * np.abs(tr[-1][1]).max()


def test_allowance_floor_and_nan():
    a = R.allowance(0.0, np.array([1.0, 0.75, 0.0], np.float32))
    assert a[0] == 2 * 2.0 ** -23 and a[1] == 2 * 2.0 ** -24 and a[2] < 1e-40
    assert R.allowance(1e-6, np.float32(1.0)) == 4e-6
    R.assert_within("ok", [1.0 + 3e-6], [1.0], 1e-6, [1.0])
    for bad in ([1.0 + 5e-6], [float("nan")]):
        with pytest.raises(AssertionError, match="ratio"):
            R.assert_within("bad", bad, [1.0], 1e-6, [1.0])


# ---- the conditions the GPU cases put on the reference alone, on the inputs they draw --------------------------------
REGS = {"none": (0.0, 0.0), "l2": (0.0, 1e-2), "l1": (1e-2, 0.0), "both": (1e-2, 1e-2)}


@pytest.mark.parametrize("reg", ["l2", "l1", "both"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_conditions_hold_on_the_drawn_inputs(kind, reg):
    """The regulariser matters (median |upd64 with - upd64 without| >= 100 allowances) and l1 meets no sign ambiguity
    (non-zero elements stay at |p| >= 1e-3, p0 = 0 with g = 0 stays exactly 0) over four steps at lr = 0.01."""
    rng = np.random.default_rng(11)
    p0, grads = R.draw_inputs(rng, 20011, 4)
    l1, l2 = REGS[reg]
    R.check_reference_conditions(kind, p0, grads, lr=0.01, l1=l1, l2=l2)


def test_reference_conditions_reject_small_parameters():
    """|p0| scaled down to [0.05, 0.15]: RMSprop at lr = 0.01 moves by 0.1 in its first step and crosses zero."""
    rng = np.random.default_rng(11)
    p0, grads = R.draw_inputs(rng, 20011, 4)
    p0 = (p0 * 0.1).astype(np.float32)
    with pytest.raises(AssertionError):
        R.check_reference_conditions("rmsprop", p0, grads, lr=0.01, l1=1e-2, l2=1e-2)
