"""Plain references for the optimizer kernels (csrc/optim.hip): torch.optim on the CPU in a chosen precision, the
regulariser added to the gradient the way BaseModel.get_regularization_loss differentiates to.  No GPU in here.

dtype = float64 is the reference; dtype = float32 on the same inputs is the yardstick of the tolerance: what an honest
float32 implementation loses against float64 (`allowance`).  Hyper-parameters enter as the float32 values the C struct
carries (mml_opt_hyper holds floats), in both precisions."""
import numpy as np
import torch

KINDS = ("sgd", "adam", "adagrad", "rmsprop")
DEFAULT_EPS = {"sgd": 0.0, "adam": 1e-8, "adagrad": 1e-10, "rmsprop": 1e-8}
STATE_KEYS = {"sgd": (), "adam": ("exp_avg", "exp_avg_sq"), "adagrad": ("sum",), "rmsprop": ("square_avg",)}


def f32(x):
    """The value a float field of mml_opt_hyper / mml_opt_tensor holds for x."""
    return float(np.float32(x))


def _optimizer(kind, p, lr, betas, eps, alpha):
    eps = DEFAULT_EPS[kind] if eps is None else eps
    if kind == "sgd":
        return torch.optim.SGD([p], lr=f32(lr), foreach=False)
    if kind == "adam":
        return torch.optim.Adam([p], lr=f32(lr), betas=(f32(betas[0]), f32(betas[1])), eps=f32(eps), foreach=False)
    if kind == "adagrad":
        return torch.optim.Adagrad([p], lr=f32(lr), eps=f32(eps), foreach=False)
    if kind == "rmsprop":
        return torch.optim.RMSprop([p], lr=f32(lr), alpha=f32(alpha), eps=f32(eps), foreach=False)
    raise NotImplementedError(kind)


def _reg_grad(p, g, l1, l2):
    """g + l1 sign(p) + 2 l2 p in p's precision (d/dp of l1 |p| + l2 p^2)."""
    if l1:
        g = g + f32(l1) * torch.sign(p)
    if l2:
        g = g + (2.0 * f32(l2)) * p
    return g


def _states(kind, opt, p):
    st = opt.state[p] if p in opt.state else {}
    out = [st[k].detach().numpy().copy() for k in STATE_KEYS[kind]]
    return out + [None] * (2 - len(out))


def dense_trajectory(kind, p0, grads, *, lr, l1=0.0, l2=0.0, betas=(0.9, 0.999), eps=None, alpha=0.99,
                     dtype=torch.float64):
    """torch.optim.{SGD, Adam, Adagrad, RMSprop} over the gradients `grads` (one array per step) from p0 with zero state.
    Returns one (p, state1, state2) per step, numpy arrays in `dtype` (a state the kind does not have is None)."""
    p = torch.tensor(np.asarray(p0), dtype=dtype).clone().requires_grad_(True)
    opt = _optimizer(kind, p, lr, betas, eps, alpha)
    out = []
    for g in grads:
        with torch.no_grad():
            p.grad = _reg_grad(p.detach(), torch.tensor(np.asarray(g), dtype=dtype), l1, l2)
        opt.step()
        out.append((p.detach().numpy().copy(), *_states(kind, opt, p)))
    return out


def masked_step(kind, p, s1, s2, g, mask, step, *, lr, l1=0.0, l2=0.0, betas=(0.9, 0.999), eps=None, alpha=0.99,
                dtype=torch.float64):
    """Step number `step` (1-based) of the dense optimizer from (p, s1, s2), applied to the rows `mask` names (bool
    [rows], or None for all); the other rows keep p and their state.  Returns (p, s1, s2) in `dtype`."""
    q = torch.tensor(np.asarray(p), dtype=dtype).clone().requires_grad_(True)
    opt = _optimizer(kind, q, lr, betas, eps, alpha)
    given = [None if s is None else torch.tensor(np.asarray(s), dtype=dtype).clone() for s in (s1, s2)]
    if kind != "sgd":
        st = {"step": torch.tensor(float(step - 1))}
        for key, s in zip(STATE_KEYS[kind], given):
            st[key] = s
        opt.state[q] = st
    with torch.no_grad():
        q.grad = _reg_grad(q.detach(), torch.tensor(np.asarray(g), dtype=dtype), l1, l2)
    opt.step()
    new = [q.detach().numpy().copy()] + _states(kind, opt, q)
    if mask is not None:
        keep = ~np.asarray(mask, bool)
        for a, old in zip(new, (p, s1, s2)):
            if a is not None:
                a[keep] = np.asarray(old)[keep].astype(a.dtype)
    return tuple(new)


def masked_trajectory(kind, p0, grads, masks, *, dtype=torch.float64, **hyper):
    """Steps 1, 2, ... of masked_step from zero state: step k moves the rows masks[k] names (None: all) with grads[k].
    The shape of dense_trajectory's result."""
    zeros = np.zeros_like(np.asarray(p0), dtype=np.float64)
    p, s1, s2 = np.asarray(p0), zeros, zeros
    out = []
    for k, (g, mask) in enumerate(zip(grads, masks)):
        p, a, b = masked_step(kind, p, s1, s2, g, mask, k + 1, dtype=dtype, **hyper)
        s1, s2 = (zeros if a is None else a), (zeros if b is None else b)
        out.append((p, a, b))
    return out


def zero_grad_replay(kind, p, m, v, from_step, to_step, *, lr, betas=(0.9, 0.999), eps=None, alpha=0.99,
                     dtype=np.float64):
    """The dense update with g = 0 over the steps (from_step[row], to_step] of every row of p [rows, E], written out in
    numpy (torch.optim's expressions with the gradient terms gone).  from_step: int per row, or one int.  Returns
    (p, m, v) in `dtype`; Adam's step size and bias correction are python floats as in torch."""
    eps = DEFAULT_EPS[kind] if eps is None else eps
    p = np.array(p, dtype=dtype)
    m = None if m is None else np.array(m, dtype=dtype)
    v = None if v is None else np.array(v, dtype=dtype)
    frm = np.broadcast_to(np.asarray(from_step, np.int64), p.shape[:1])
    T = dtype
    b1, b2, al, lr_ = f32(betas[0]), f32(betas[1]), f32(alpha), f32(lr)
    for j in range(int(frm.min()) + 1 if frm.size else to_step + 1, int(to_step) + 1):
        on = frm < j
        if not on.any():
            continue
        if kind == "adam":
            m[on] = m[on] + T(1.0 - b1) * (T(0.0) - m[on])            # exp_avg.lerp_(0, 1 - beta1)
            v[on] = v[on] * T(b2)
            step_size = lr_ / (1.0 - b1 ** j)
            denom = np.sqrt(v[on]) / T(np.sqrt(1.0 - b2 ** j)) + T(f32(eps))
            p[on] = p[on] - T(step_size) * (m[on] / denom)
        elif kind == "rmsprop":
            m[on] = m[on] * T(al)                                     # square_avg decays, p -= lr * 0 / (..)
        # sgd / adagrad: a zero gradient changes nothing
    return p, m, v


def draw_inputs(rng, shape, steps, zero_share=0.05, grad_share=0.3):
    """Inputs without sign ambiguity under l1: |p0| in [0.5, 1.5] with random signs, `zero_share` of the elements exactly
    0 with a zero gradient in every step (they must stay exactly 0), the other gradients standard normal with a share
    of exact zeros (the scatter leaves most of a table's gradient zero; with grad_share below one half the MEDIAN element
    has g = 0, where Adam, Adagrad and RMSprop move by the regulariser alone -- next to a gradient their first step is
    lr sign(g) with or without it).  float32 arrays: (p0, [g_1 .. g_steps])."""
    p0 = (rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    dead = rng.random(shape) < zero_share
    p0[dead] = 0.0
    grads = []
    for _ in range(steps):
        g = (rng.standard_normal(shape) * (rng.random(shape) < grad_share)).astype(np.float32)
        g[dead] = 0.0
        grads.append(g)
    return p0, grads


def allowance(e32, before):
    """What a float32 kernel may be off by per element: four times the float32 reference's own worst distance from the
    float64 one (FMA contraction, the lerp form of Adam's first moment, extremes over millions of elements), and never
    below two spacings of the value the result is rounded next to (an update below the spacing is quantised)."""
    return np.maximum(4.0 * float(e32), 2.0 * np.spacing(np.abs(np.asarray(before, np.float32))).astype(np.float64))


def e32_of(tr32, tr64, p0):
    """Per step: (max |upd32 - upd64| of p, max |s1_32 - s1_64|, max |s2_32 - s2_64|) of two dense_trajectory results
    over the same inputs; the update of step k is p_k - p_{k-1} of the trajectory's own p."""
    out = []
    b32 = np.asarray(p0, np.float32).astype(np.float64)
    b64 = np.asarray(p0, np.float64)
    for (p32, a32, c32), (p64, a64, c64) in zip(tr32, tr64):
        p32 = p32.astype(np.float64)
        row = [float(np.abs((p32 - b32) - (p64 - b64)).max()) if p64.size else 0.0]
        for s32, s64 in ((a32, a64), (c32, c64)):
            row.append(0.0 if s64 is None or not s64.size else float(np.abs(s32.astype(np.float64) - s64).max()))
        out.append(tuple(row))
        b32, b64 = p32, p64
    return out


def reference_case(kind, p0, grads, *, l1=0.0, l2=0.0, **hyper):
    """The float64 trajectory of a case and, per step, e32_of(float32 trajectory, it) -- after the conditions on the
    reference alone: elements with p0 = 0 and g = 0 stay exactly 0, every other element stays at |p| >= 1e-3 (no sign
    ambiguity under l1), and a regulariser matters: per step, the median over the non-zero elements of
    |upd64 with - upd64 without| / allowance is at least 100."""
    p0 = np.asarray(p0, np.float32)
    tr64 = dense_trajectory(kind, p0, grads, l1=l1, l2=l2, dtype=torch.float64, **hyper)
    tr32 = dense_trajectory(kind, p0, grads, l1=l1, l2=l2, dtype=torch.float32, **hyper)
    e32 = e32_of(tr32, tr64, p0)
    dead = p0 == 0
    assert all(not np.asarray(g)[dead].any() for g in grads), "an element with p0 = 0 has a gradient"
    for p64, _, _ in tr64:
        assert not p64[dead].any(), "an element with p0 = 0 and g = 0 moved in the reference"
        assert p64.size == 0 or dead.all() or np.abs(p64[~dead]).min() >= 1e-3, "an element came within 1e-3 of zero"
    if (l1 or l2) and not dead.all():
        plain = dense_trajectory(kind, p0, grads, dtype=torch.float64, **hyper)
        b_reg = b_plain = p0.astype(np.float64)
        for k, ((p_reg, _, _), (p_plain, _, _)) in enumerate(zip(tr64, plain)):
            diff = np.abs((p_reg - b_reg) - (p_plain - b_plain))[~dead]
            weight = float(np.median(diff / allowance(e32[k][0], b_reg)[~dead]))
            assert weight >= 100, f"{kind} step {k + 1}: the regulariser is worth only {weight:.1f} allowances"
            b_reg, b_plain = p_reg, p_plain
    return tr64, e32


def check_reference_conditions(kind, p0, grads, **kw):
    reference_case(kind, p0, grads, **kw)


def assert_within(tag, got, ref, e32, before):
    """|got - ref| <= allowance(e32, before) for every element (NaN fails); the message names e32, the worst error and
    their ratio, which is returned."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not ref.size:
        return 0.0
    err = np.abs(got - ref)
    bad = ~(err <= allowance(e32, before))
    worst = float(np.nanmax(err)) if not np.isnan(err).all() else float("nan")
    ratio = worst / e32 if e32 > 0 else (0.0 if worst == 0 else float("inf"))
    assert not bad.any(), (f"{tag}: e32 {e32:.3e}, kernel's worst error {worst:.3e}, ratio {ratio:.2f}; "
                           f"{int(bad.sum())} of {bad.size} elements outside the allowance")
    return ratio
