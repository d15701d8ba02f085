"""References, input builders and the comparator of the kernel-parity tests for the APG, SNR, ESMM / ESCM and DomainBN
kernels (tests/test_model_kernel_refs_cpu.py proves them on the host, tests/test_model_kernels_gpu.py uses them on the
device).  A plain helper module: no fixtures, no GPU.

  ref64_*    float64 numpy references written from the reference project's formulas (model/apg.py:77-104,
             model/snr_trans.py:38-50, model/mssm.py:26-58, model/esmm.py:58-62 + model/basemodel.py:294-296,
             model/escm.py:98-112 + model/basemodel.py:284-292, model/utils.py:553-636).  They read the float32 inputs
             exactly as uploaded and return every output together with, for every output that is a sum, the
             per-element sum of the absolute values of its terms ("sumabs").
  model32_*  float32 numpy restatements of the arithmetic the kernels do, with named mutations.  They exist so that the
             CPU file can prove that comparator + inputs notice each mutation; they are never a reference for the GPU.
  build_*    seeded input builders; each returns the inputs and a census of the branches they exercise.
  assert_close_terms   |got - ref| <= tol * sumabs element by element, NaN positions identical; never a max-norm.
"""
import numpy as np

F32 = np.float32
F64 = np.float64
BCE_FLOOR = float(F32(1e-12))  # torch's (and the kernels') float32 constant in the BCE gradient denominator
IPW_FLOOR = 1e-6
IPW_CLIP = 15.0
SNR_BETA, SNR_GAMMA, SNR_EPS = 0.9, -0.1, 1.1

RATIOS = {}  # worst err / (tol * sumabs) seen per `what` prefix (the text before the first ':')


# ---------------------------------------------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------------------------------------------
def assert_close_terms(got, ref, sumabs, tol, what):
    """Element-wise |got - ref| <= tol * sumabs; NaN positions must coincide exactly.  Returns the worst
    err / (tol * sumabs) (0 where both are 0) and records it in RATIOS; the failure message carries it with its index."""
    got = np.asarray(got, dtype=F64)
    ref = np.asarray(ref, dtype=F64)
    sumabs = np.broadcast_to(np.asarray(sumabs, dtype=F64), ref.shape)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    gn, rn = np.isnan(got), np.isnan(ref)
    if not np.array_equal(gn, rn):
        idx = np.argwhere(gn != rn)[0]
        raise AssertionError(f"{what}: NaN positions differ, first at {tuple(idx)}: got {got[tuple(idx)]!r}, "
                             f"reference {ref[tuple(idx)]!r} ({int((gn != rn).sum())} positions)")
    ok = ~rn
    with np.errstate(invalid="ignore"):
        same = ok & (got == ref)  # (covers equal infinities)
        err = np.where(same | ~ok, 0.0, np.abs(got - ref))
    bound = np.where(ok, tol * np.abs(sumabs), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound)  # err > 0 over a zero bound -> inf
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    worst = float(ratio.max()) if ratio.size else 0.0
    key = what.split(":")[0]
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    if worst > 1.0:
        idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.ndim else ()
        raise AssertionError(f"{what}: worst err / (tol * sumabs) = {worst:.4g} at {tuple(int(i) for i in idx)}: got "
                             f"{got[idx]!r}, reference {ref[idx]!r}, sumabs {sumabs[idx]!r}, tol {tol:g} "
                             f"({int((ratio > 1.0).sum())} of {ratio.size} elements outside)")
    return worst


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------
# APG: z_b = [o1_b (x) s_b | o1_b | s_b | 0],  o2_b = o1_b @ reshape(Wkk s_b + bkk, [k, k]) + Wb s_b
# ---------------------------------------------------------------------------------------------------------------
def build_apg(B, k, E, seed):
    rng = np.random.default_rng(seed)
    inp = dict(o1=rng.standard_normal((B, k)).astype(F32), s=rng.standard_normal((B, E)).astype(F32),
               dz=rng.standard_normal((B, k * E + k)).astype(F32), prior=rng.standard_normal((B, k)).astype(F32))
    census = dict(k_ne_E=k != E, elements_fwd=B * (k * E + k + E), elements_bwd=B * k)
    return inp, census


def build_apg_weights(k, E, seed):
    rng = np.random.default_rng(seed)
    R = k * E + k + E
    inp = dict(Wkk=rng.standard_normal((k * k, E)).astype(F32), bkk=rng.standard_normal(k * k).astype(F32),
               Wb=rng.standard_normal((k, E)).astype(F32), dWcat=rng.standard_normal((R, k)).astype(F32),
               pWkk=rng.standard_normal((k * k, E)).astype(F32), pbkk=rng.standard_normal(k * k).astype(F32),
               pWb=rng.standard_normal((k, E)).astype(F32))
    return inp, dict(k=k, E=E, rows=R)


def ref64_apg_features_fwd(o1, s, Kf):
    """[B, Kf] float64.  A product of two float32 is exact in float64, so .astype(float32) of this IS the float32 product."""
    o1, s = o1.astype(F64), s.astype(F64)
    B, k = o1.shape
    E = s.shape[1]
    z = np.zeros((B, Kf), F64)
    z[:, :k * E] = (o1[:, :, None] * s[:, None, :]).reshape(B, k * E)
    z[:, k * E:k * E + k] = o1
    z[:, k * E + k:k * E + k + E] = s
    return z


def ref64_apg_features_bwd(dz, s, k, prior=None):
    """do1[b, i] = sum_e dz[b, iE + e] s[b, e] + dz[b, kE + i] (+ prior).  Returns (do1, sumabs)."""
    dz, s = dz.astype(F64), s.astype(F64)
    B, E = s.shape
    prod = dz[:, :k * E].reshape(B, k, E) * s[:, None, :]
    tail = dz[:, k * E:k * E + k]
    out, sa = prod.sum(2) + tail, np.abs(prod).sum(2) + np.abs(tail)
    if prior is not None:
        out, sa = out + prior.astype(F64), sa + np.abs(prior.astype(F64))
    return out, sa


def ref64_apg_pack(Wkk, bkk, Wb, k, E):
    """W_cat [kE + k + E, k]: row iE+e, column j <- Wkk[ik+j, e]; row kE+i <- bkk[ik+j]; row kE+k+e <- Wb[j, e]."""
    Wc = np.zeros((k * E + k + E, k), F64)
    Wc[:k * E] = Wkk.astype(F64).reshape(k, k, E).transpose(0, 2, 1).reshape(k * E, k)
    Wc[k * E:k * E + k] = bkk.astype(F64).reshape(k, k)
    Wc[k * E + k:] = Wb.astype(F64).T
    return Wc


def ref64_apg_unpack(dWcat, k, E, priors=(None, None, None)):
    """(dWkk, dbkk, dWb), each (value, sumabs): the inverse re-layout, added to a prior where one is given."""
    d = dWcat.astype(F64)
    parts = [d[:k * E].reshape(k, E, k).transpose(0, 2, 1).reshape(k * k, E), d[k * E:k * E + k].reshape(k * k),
             d[k * E + k:].T.copy()]
    out = []
    for v, p in zip(parts, priors):
        if p is None:
            out.append((v, np.abs(v)))
        else:
            out.append((v + p.astype(F64), np.abs(v) + np.abs(p.astype(F64))))
    return out


def ref64_apg_generated(o1, s, Wkk, bkk, Wb):
    """The reference's per-sample generated-weight form (model/apg.py:78-80, :101) without the bias-generator's own bias:
    o2_b = o1_b @ reshape(Wkk s_b + bkk, [k, k]) + Wb s_b.  Returns (o2, sumabs over the expanded products)."""
    o1, s, Wkk, bkk, Wb = (a.astype(F64) for a in (o1, s, Wkk, bkk, Wb))
    B, k = o1.shape
    o2, sa = np.zeros((B, k)), np.zeros((B, k))
    aW, ab, aWb = np.abs(Wkk), np.abs(bkk), np.abs(Wb)
    for b in range(B):
        Wgen = (Wkk @ s[b] + bkk).reshape(k, k)
        o2[b] = o1[b] @ Wgen + Wb @ s[b]
        sa[b] = np.abs(o1[b]) @ (aW @ np.abs(s[b]) + ab).reshape(k, k) + aWb @ np.abs(s[b])
    return o2, sa


def model32_apg_features_fwd(o1, s, Kf, prior, mutate=None):
    """`prior` is what the buffer held before (the GPU test's sentinel)."""
    B, k = o1.shape
    E = s.shape[1]
    z = prior.astype(F32).copy()
    if mutate == "swap_o1_s":  # o1[e] * s[i]
        i, e = np.divmod(np.arange(k * E), E)
        z[:, :k * E] = o1[:, e % k] * s[:, i % E]
    else:
        z[:, :k * E] = (o1[:, :, None] * s[:, None, :]).reshape(B, k * E)
    z[:, k * E:k * E + k] = o1
    z[:, k * E + k:k * E + k + E] = s
    if mutate != "pad_unwritten":
        z[:, k * E + k + E:] = 0
    return z


def model32_apg_features_bwd(dz, s, k, prior, accumulate, mutate=None):
    B, E = s.shape
    acc = np.zeros((B, k), F32) if mutate == "drop_dz_tail" else dz[:, k * E:k * E + k].astype(F32).copy()
    for e in range(E - 1 if mutate == "E_minus_1" else E):
        acc = (acc + dz[:, e:k * E:E] * s[:, e:e + 1]).astype(F32)
    if accumulate and mutate != "ignore_accumulate":
        acc = (prior + acc).astype(F32)
    return acc


def model32_apg_pack(Wkk, bkk, Wb, k, E, mutate=None):
    Wc = np.zeros((k * E + k + E, k), F32)
    W3 = Wkk.reshape(k, k, E)
    if mutate == "wkk_ji":
        W3 = W3.transpose(1, 0, 2)
    Wc[:k * E] = W3.transpose(0, 2, 1).reshape(k * E, k)
    Wc[k * E:k * E + k] = bkk.reshape(k, k).T if mutate == "bkk_T" else bkk.reshape(k, k)
    Wc[k * E + k:] = Wb.reshape(E, k) if mutate == "wb_Ek" else Wb.T
    return Wc


def model32_apg_unpack(dWcat, k, E, priors, flags, mutate=None):
    """dir 1 over the priors (pWkk, pbkk, pWb) with flags (acc_kk, acc_bkk, acc_wb)."""
    d3 = dWcat[:k * E].reshape(k, E, k).transpose(0, 2, 1)
    if mutate == "wkk_ji":
        d3 = d3.transpose(1, 0, 2)
    db = dWcat[k * E:k * E + k]
    parts = [d3.reshape(k * k, E), (db.T if mutate == "bkk_T" else db).reshape(k * k),
             dWcat[k * E + k:].reshape(k, E) if mutate == "wb_Ek" else dWcat[k * E + k:].T]
    out = []
    for name, v, p, f in zip(("kk", "bkk", "wb"), parts, priors, flags):
        if mutate == "ignore_acc_" + name:
            f = 0
        out.append((p + v).astype(F32) if f else v.astype(F32).copy())
    return out


# ---------------------------------------------------------------------------------------------------------------
# SNR / MSSM hard-concrete gate
# ---------------------------------------------------------------------------------------------------------------
SNR_SPECIAL_U = (0.97, 0.02, 0.3, 1 - 1e-6, 0.5, 1e-6, 0.8)  # at one (alpha >= 1) / dead / live / extremes


def ref64_snr_z(u, alpha, beta=SNR_BETA, gamma=SNR_GAMMA, eps=SNR_EPS):
    """model/snr_trans.py:40-43.  Returns z, dz/du, dz/dalpha, s_ (the stretched value before the two clamps); the
    constants are read at their float32 values, as the kernel receives them."""
    u = np.asarray(u).astype(F64)
    a, beta, gamma, eps = float(F32(alpha)), float(F32(beta)), float(F32(gamma)), float(F32(eps))
    logit = np.log(u) - np.log1p(-u) + np.log(a) / beta
    s = 1.0 / (1.0 + np.exp(-logit))
    sb = s * (eps - gamma) + gamma
    pos = (sb > 0).astype(F64) * sb                     # (s_ > 0).float() * s_
    z = (pos > 1).astype(F64) + (pos <= 1).astype(F64) * pos
    live = (sb > 0) & (sb <= 1)
    ds = np.where(live, (eps - gamma) * s * (1 - s), 0.0)
    return z, ds * (1 / u + 1 / (1 - u)), ds / (a * beta), sb


def build_snr(n_blocks, rows, cols, zw, alpha, seed):
    """u [n_blocks * zw] (the special values first, then uniform(0.001, 0.999), the last one live), M / dW
    [n_blocks, rows, cols] standard normal, non-zero priors.  No s_ within 1e-3 of 0 or 1 (u is nudged by x1.01 until that holds)."""
    assert zw in (1, cols)
    rng = np.random.default_rng(seed)
    nu = n_blocks * zw
    u = rng.uniform(0.001, 0.999, nu)
    sp = np.array(SNR_SPECIAL_U[:nu])
    u[:len(sp)] = sp
    if nu > 1:  # the last coefficient sits at s = 0.5 (live at every alpha): the last block contributes to dalpha
        u[-1] = 1.0 / (1.0 + np.exp(np.log(alpha) / SNR_BETA))
    u = u.astype(F32)
    for _ in range(40):
        sb = ref64_snr_z(u, alpha)[3]
        near = (np.abs(sb) < 1e-3) | (np.abs(sb - 1) < 1e-3)
        if not near.any():
            break
        u[near] = np.minimum(u[near] * F32(1.01), F32(1 - 1e-6))
    assert not near.any()
    sb = ref64_snr_z(u, alpha)[3]
    inp = dict(u=u, alpha=np.array([alpha], F32), M=rng.standard_normal((n_blocks, rows, cols)).astype(F32),
               dW=rng.standard_normal((n_blocks, rows, cols)).astype(F32),
               prior_du=rng.standard_normal(nu).astype(F32), prior_dalpha=rng.standard_normal(1).astype(F32))
    census = dict(dead=int((sb <= 0).sum()), one=int((sb > 1).sum()), live=int(((sb > 0) & (sb <= 1)).sum()), n=nu)
    return inp, census


def _snr_expand(v, n_blocks, rows, cols, zw):
    """per-coefficient values -> [n_blocks, rows, cols] (zw = 1: one per block; zw = cols: one per output column)"""
    v = v.reshape(n_blocks, 1, zw)
    return np.broadcast_to(v, (n_blocks, rows, cols))


def ref64_snr_fwd(u, alpha, M, zw):
    """W = z * M.  Returns (W, |M|, z expanded): the check is |W - z M| <= 1e-5 |M|."""
    nb, rows, cols = M.shape
    z = _snr_expand(ref64_snr_z(u, alpha[0])[0], nb, rows, cols, zw)
    return z * M.astype(F64), np.abs(M.astype(F64)), z


def ref64_snr_bwd(dW, M, u, alpha, zw, prior_du=None, prior_dalpha=None):
    """du_c = <dW, M>_c dz/du_c, dalpha = sum_c <dW, M>_c dz/dalpha_c (c: block for zw = 1, (block, column) else), each
    plus its prior when given.  Returns du, du_sumabs, dalpha, dalpha_sumabs."""
    nb, rows, cols = M.shape
    _, dzu, dza, _ = ref64_snr_z(u, alpha[0])
    gm = dW.astype(F64) * M.astype(F64)
    if zw == 1:
        dot, adot = gm.sum((1, 2)), np.abs(gm).sum((1, 2))
    else:
        dot, adot = gm.sum(1).reshape(-1), np.abs(gm).sum(1).reshape(-1)
    du, du_sa = dot * dzu, adot * np.abs(dzu)
    da, da_sa = np.array([(dot * dza).sum()]), np.array([(adot * np.abs(dza)).sum()])
    if prior_du is not None:
        du, du_sa = du + prior_du.astype(F64), du_sa + np.abs(prior_du.astype(F64))
    if prior_dalpha is not None:
        da, da_sa = da + prior_dalpha.astype(F64), da_sa + np.abs(prior_dalpha.astype(F64))
    return du, du_sa, da, da_sa


def model32_snr_z(u, alpha, mutate=None):
    a, b, g, e = F32(alpha), F32(SNR_BETA), F32(SNR_GAMMA), F32(SNR_EPS)
    la = np.log(a) * b if mutate == "log_alpha_times_beta" else np.log(a) / b
    logit = (np.log(u) - np.log(F32(1) - u) + la).astype(F32)
    s = (F32(1) / (F32(1) + np.exp(-logit))).astype(F32)
    sb = (s * (e - g) + g).astype(F32)
    live = (sb > 0) if mutate == "deriv_above_saturation" else (sb > 0) & (sb <= 1)
    z = np.where(sb <= 0, F32(0), np.where(sb > 1, F32(1), sb)).astype(F32)
    ds = np.where(live, (e - g) * s * (F32(1) - s), F32(0)).astype(F32)
    return z, (ds * (F32(1) / u + F32(1) / (F32(1) - u))).astype(F32), (ds / (a * b)).astype(F32)


def model32_snr_fwd(u, alpha, M, zw, mutate=None):
    nb, rows, cols = M.shape
    z = model32_snr_z(u, alpha[0], mutate)[0]
    if zw > 1 and mutate == "zw_col_div":  # element i of the block read as column i / zw
        idx = np.minimum(np.arange(rows * cols) // zw, zw - 1)
        return (z.reshape(nb, zw)[:, idx].reshape(nb, rows, cols) * M).astype(F32)
    return (_snr_expand(z, nb, rows, cols, zw) * M).astype(F32)


def model32_snr_bwd(dW, M, u, alpha, zw, prior_du, prior_dalpha, acc_u, acc_alpha, want_du=True, mutate=None):
    nb, rows, cols = M.shape
    _, dzu, dza = model32_snr_z(u, alpha[0], mutate)
    gm = (dW * M).astype(F32)
    dot = gm.sum((1, 2), dtype=F32) if zw == 1 else gm.sum(1, dtype=F32).reshape(-1)
    du = None
    if want_du:
        du = (dot * (dza if mutate == "du_with_dz_dalpha" else dzu)).astype(F32)
        if acc_u and mutate != "acc_u_ignored":
            du = (prior_du + du).astype(F32)
    part = (dot * dza).astype(F32).reshape(nb, -1).sum(1, dtype=F32)
    if mutate == "dalpha_misses_last_block":
        part = part[:-1]
    da = np.array([part.sum(dtype=F32)], F32)
    if acc_alpha:
        da = (prior_dalpha + da).astype(F32)
    return du, da


# ---------------------------------------------------------------------------------------------------------------
# ESMM / ESCM
# ---------------------------------------------------------------------------------------------------------------
ESCM_SATURATIONS = ((0.0, 0.5), (1.0, 0.5), (0.5, 0.0), (0.5, 1.0), (1.0, 1.0), (0.0, 0.0))


def _bce64(p, y):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -(y * np.maximum(np.log(p), -100.0) + (1 - y) * np.maximum(np.log1p(-p), -100.0))


def _bce_grad64(p, y):
    return (p - y) / np.maximum((1 - p) * p, BCE_FLOOR)


def build_escm(B, npos, seed=None):
    """Probabilities and labels for both combine kernels.  c and v independently: half sigmoid(3 normal), half
    log-uniform 10^(-9 u); the first min(6, B // 4) rows are exact saturations; y0 has exactly min(npos, B) ones,
    y1 = y0 * Bernoulli(.5).  No row within 1e-3 (relative) of a branch threshold: c N = 1e-6, 1 / (c N) = 15,
    (1 - p) p = 1e-12 for p in {c, v, c v}; offending rows are nudged by x1.01, none is ever excluded."""
    rng = np.random.default_rng(B + npos if seed is None else seed)

    def draw():
        return np.where(rng.random(B) < 0.5, 10.0 ** (-9 * rng.random(B)),
                        1 / (1 + np.exp(-3 * rng.standard_normal(B)))).astype(F32)
    c, v = draw(), draw()
    for i, (a, b) in enumerate(ESCM_SATURATIONS[:min(len(ESCM_SATURATIONS), B // 4)]):
        c[i], v[i] = a, b
    y0 = np.zeros(B, F32)
    y0[rng.permutation(B)[:min(npos, B)]] = 1
    y1 = (y0 * (rng.random(B) < 0.5)).astype(F32)
    for _ in range(40):
        near = escm_near_threshold(c, v, y0)
        if not near.any():
            break
        c[near] = (c[near] * F32(1.01)).astype(F32)
        v[near] = (v[near] * F32(1.01)).astype(F32)
    assert not escm_near_threshold(c, v, y0).any()
    inp = dict(praw=np.stack([c, v], 1), y=np.stack([y0, y1], 1),
               dout2=rng.standard_normal((B, 2)).astype(F32), dout3=rng.standard_normal((B, 3)).astype(F32))
    return inp, escm_census(c, y0)


def escm_near_threshold(c, v, y0):
    c64, v64, N = c.astype(F64), v.astype(F64), float(y0.astype(F64).sum())
    near = np.zeros(len(c), bool)
    if N > 0:
        near |= np.abs(c64 * N / IPW_FLOOR - 1) < 1e-3
        near |= np.abs(1 / np.maximum(c64 * N, 1e-300) / IPW_CLIP - 1) < 1e-3
    for p in (c64, v64, c64 * v64):
        near |= np.abs((1 - p) * p / BCE_FLOOR - 1) < 1e-3
    return near


def escm_census(c, y0):
    """positive rows (y0 = 1) per counterfactual-IPW regime"""
    c64, N = c.astype(F64), float(y0.astype(F64).sum())
    pos = y0 > 0
    floored = c64 * N <= IPW_FLOOR
    with np.errstate(divide="ignore"):
        clipped = ~floored & (1 / (c64 * N) > IPW_CLIP) if N > 0 else np.zeros(len(c), bool)
    return dict(N=int(N), unclipped=int((pos & ~floored & ~clipped).sum()), clipped=int((pos & clipped).sum()),
                floored=int((pos & floored).sum()), pos_beyond_1024=int(pos[1024:].sum()), neg=int((~pos).sum()))


def ref64_esmm(praw, y=None, dout=None):
    """model/esmm.py:58-62: out = [ctr, ctr cvr]; loss = BCE_sum(out0, y0) + BCE_sum(out1, y1) (basemodel.py:294-296);
    draw = d loss / d [ctr, cvr] (or the chain rule of `dout`).  Returns a dict: pout, loss, draw, draw_sumabs."""
    c, v = praw[:, 0].astype(F64), praw[:, 1].astype(F64)
    r = dict(pout=np.stack([c, c * v], 1), loss=None, draw=None, draw_sumabs=None)
    if y is not None:
        y0, y1 = y[:, 0].astype(F64), y[:, 1].astype(F64)
        r["loss"] = float(_bce64(c, y0).sum() + _bce64(c * v, y1).sum())
        g0, g1 = _bce_grad64(c, y0), _bce_grad64(c * v, y1)
    elif dout is not None:
        g0, g1 = dout[:, 0].astype(F64), dout[:, 1].astype(F64)
    else:
        return r
    r["draw"] = np.stack([g0 + g1 * v, g1 * c], 1)
    r["draw_sumabs"] = np.stack([np.abs(g0) + np.abs(g1 * v), np.abs(g1 * c)], 1)
    return r


def ref64_escm(praw, y=None, dout=None, cf_w=0.1, global_w=1.0):
    """model/escm.py:98-112 + basemodel.py:284-292: out = [ctr, cvr, ctr cvr];
    loss = BCE_sum(ctr, y0) + cf_w mean_b(L1 ips_b y0_b) + global_w BCE_sum(ctr cvr, y1), L1 = BCE_sum(cvr, y1),
    ips_b = clip(1 / max(ctr_b N, 1e-6), -15, 15) B, N = sum y0 -- the gradient flows through ips."""
    c, v = praw[:, 0].astype(F64), praw[:, 1].astype(F64)
    cf, gw = float(F32(cf_w)), float(F32(global_w))
    r = dict(pout=np.stack([c, v, c * v], 1), loss=None, draw=None, draw_sumabs=None)
    if y is None:
        if dout is not None:
            d0, d1, d2 = (dout[:, i].astype(F64) for i in range(3))
            r["draw"] = np.stack([d0 + d2 * v, d1 + d2 * c], 1)
            r["draw_sumabs"] = np.stack([np.abs(d0) + np.abs(d2 * v), np.abs(d1) + np.abs(d2 * c)], 1)
        return r
    y0, y1 = y[:, 0].astype(F64), y[:, 1].astype(F64)
    B, N = len(c), y0.sum()
    L0, L1, L2 = _bce64(c, y0).sum(), _bce64(v, y1).sum(), _bce64(c * v, y1).sum()
    rr = 1 / np.maximum(c * N, IPW_FLOOR)
    ips = np.clip(rr, -IPW_CLIP, IPW_CLIP) * B
    r["loss"] = float(L0 + cf * np.mean(L1 * ips * y0) + gw * L2)
    S = (y0 * ips).sum() / B
    inside = (c * N > IPW_FLOOR) & (rr <= IPW_CLIP)
    dips = np.where(inside, -N * rr * rr, 0.0)
    g2 = gw * _bce_grad64(c * v, y1)
    t0 = [_bce_grad64(c, y0), cf * L1 * y0 * dips, g2 * v]
    t1 = [cf * S * _bce_grad64(v, y1), g2 * c]
    r["draw"] = np.stack([sum(t0), sum(t1)], 1)
    r["draw_sumabs"] = np.stack([sum(np.abs(t) for t in t0), sum(np.abs(t) for t in t1)], 1)
    return r


def _bce32(p, y):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (-(y * np.maximum(np.log(p), F32(-100)) + (F32(1) - y) * np.maximum(np.log1p(-p), F32(-100)))).astype(F32)


def _bce32_noclamp(p, y):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (-(y * np.log(p) + (F32(1) - y) * np.log1p(-p))).astype(F32)


def _bce_grad32(p, y):
    return ((p - y) / np.maximum((F32(1) - p) * p, F32(1e-12))).astype(F32)


def _wave0(a):
    """what a 1024-thread workgroup keeps when only its first wave's partial survives: rows b with b % 1024 < 64"""
    return a[(np.arange(len(a)) % 1024) < 64]


def model32_esmm(praw, y=None, dout=None, want_draw=True, want_loss=True, prior_pout=None, prior_draw=None, mutate=None):
    """float32 restatement; the priors are what the output buffers held before (rows a mutation skips keep them)."""
    c, v = praw[:, 0], praw[:, 1]
    B = len(c)
    rows = slice(0, min(B, 1024)) if mutate == "skip_rows_ge_1024" else slice(0, B)
    p1 = (c * v).astype(F32)
    r = dict(pout=(np.full((B, 2), np.nan, F32) if prior_pout is None else prior_pout.copy()), loss=None, draw=None)
    r["pout"][rows] = np.stack([c, p1], 1)[rows]
    if y is not None:
        y0, y1 = y[:, 0], y[:, 1]
        bce = _bce32_noclamp if mutate == "loss_without_clamp" else _bce32
        terms = (bce(c, y0) + bce(p1, y1)).astype(F32)[rows]
        if mutate == "wave0_only":
            terms = _wave0(terms)
        if want_loss:
            r["loss"] = F32(terms.sum(dtype=F32))
        g0, g1 = _bce_grad32(c, y0), _bce_grad32(p1, y1)
    elif dout is not None:
        g0, g1 = dout[:, 0], dout[:, 1]
    else:
        return r
    if want_draw:
        d0 = g0 if mutate == "dctr_without_g1v" else (g0 + g1 * v).astype(F32)
        r["draw"] = np.full((B, 2), np.nan, F32) if prior_draw is None else prior_draw.copy()
        r["draw"][rows] = np.stack([d0, (g1 * c).astype(F32)], 1)[rows]
    return r


def model32_escm(praw, y=None, dout=None, cf_w=0.1, global_w=1.0, want_draw=True, want_loss=True, mutate=None):
    c, v = praw[:, 0], praw[:, 1]
    cf, gw = F32(cf_w), F32(global_w)
    p2 = (c * v).astype(F32)
    r = dict(pout=np.stack([c, v, p2], 1), loss=None, draw=None)
    if y is None:
        if dout is not None and want_draw:
            r["draw"] = np.stack([dout[:, 0] + dout[:, 2] * v, dout[:, 1] + dout[:, 2] * c], 1).astype(F32)
        return r
    y0, y1 = y[:, 0], y[:, 1]
    N = F32((y0[:1024] if mutate == "N_first_1024_rows" else y0).sum(dtype=F32))
    L0, L1, L2 = (F32(_bce32(p, t).sum(dtype=F32)) for p, t in ((c, y0), (v, y1), (p2, y1)))
    ps = np.maximum(c * N, F32(1e-6))
    rr = (F32(1) / ps).astype(F32)
    clip = np.clip(rr, F32(-15), F32(15))
    S = F32((clip if mutate == "S_without_y0" else y0 * clip).sum(dtype=F32))
    if want_loss:
        r["loss"] = F32((cf * L0 if mutate == "cf_w_on_L0" else L0) + cf * (L1 * S) + gw * L2)
    if not want_draw:
        return r
    inside = np.ones(len(c), bool) if mutate == "dips_when_clipped" else (c * N > F32(1e-6)) & (rr <= F32(15))
    with np.errstate(over="ignore", invalid="ignore"):
        dips = np.where(inside, -N * rr * rr, F32(0)).astype(F32)
        g0, g1 = _bce_grad32(c, y0), _bce_grad32(v, y1)
        g2 = _bce_grad32(p2, y1) if mutate == "g2_without_global_w" else (gw * (p2 - y1) / np.maximum(
            (F32(1) - p2) * p2, F32(1e-12))).astype(F32)
        if mutate == "cf_w_on_L0":
            g0 = (cf * g0).astype(F32)
        d0 = (g0 + cf * L1 * y0 * dips + g2 * v).astype(F32)
        d1 = (g2 * c).astype(F32) if mutate == "draw1_without_cf_S_g1" else (cf * S * g1 + g2 * c).astype(F32)
    r["draw"] = np.stack([d0, d1], 1)
    return r


# ---------------------------------------------------------------------------------------------------------------
# DomainBatchNorm (model/utils.py:553-636)
# ---------------------------------------------------------------------------------------------------------------
def build_domain_bn(B, n, D, seed, degenerate=False, soft=False):
    """x ~ N(d, 1.5) + column offsets; masks mostly one-hot plus one all-zero row (arg-max tie -> domain 0) and one row
    with two equal maxima (the first wins); `soft` adds a few rows of non-one-hot weights (eval); `degenerate` leaves the
    last domain empty and gives the one before exactly one sample.  Priors are non-trivial."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, n)) * 1.5 + rng.standard_normal(n)).astype(F32)
    dom = rng.integers(0, D, B)
    if degenerate:  # row 0 alone in domain D - 2, the others alternate over the first D - 2 domains, none in D - 1
        dom[0] = D - 2
        dom[1:] = np.arange(B - 1) % (D - 2)
    else:
        dom[:D] = np.arange(D)  # every domain has samples
        dom[D:2 * D] = np.arange(D)
    mask = np.zeros((B, D), F32)
    mask[np.arange(B), dom] = 1
    zero_row, tie_row = B - 1, B - 2
    mask[zero_row] = 0                      # argmax of an all-zero row: 0
    mask[tie_row] = 0
    mask[tie_row, D - 3 if degenerate else D - 2] = 0.5  # two equal maxima: the first wins
    mask[tie_row, D - 4 if degenerate else D - 1] = 0.5
    soft_rows = []
    if soft:
        soft_rows = [3 * D, 3 * D + 1, 3 * D + 2]
        w = np.array([0.25, 0.75] + [0.0] * (D - 2), F32)
        for i, r_ in enumerate(soft_rows):
            mask[r_] = np.roll(w, i)
    arg = np.argmax(mask, 1)
    pop_mean = rng.standard_normal((D, n)).astype(F32)
    pop_var = (10.0 ** rng.uniform(-3, 0.6, (D, n))).astype(F32)
    cnt = np.bincount(arg, minlength=D)
    census = dict(counts=cnt.tolist(), empty=int((cnt == 0).sum()), single=int((cnt == 1).sum()), zero_row=zero_row,
                  tie_row=tie_row, tie_first=int(arg[tie_row]), soft_rows=soft_rows)
    return dict(x=x, mask=mask, pop_mean=pop_mean, pop_var=pop_var), census


def ref64_domain_bn_update(x, mask, pop_mean, pop_var, decay):
    """pop[d] = pop[d] decay + stat(x[argmax(mask) == d]) (1 - decay), stat = mean / UNBIASED variance, evaluated for
    every domain (utils.py:582-584, :622-624: both branches of the torch.where run), so an empty domain becomes NaN and
    a one-sample domain's variance does.  Returns mean, mean_sumabs, var, var_sumabs."""
    x64 = x.astype(F64)
    D = mask.shape[1]
    arg = np.argmax(mask, axis=1)  # numpy and torch: first maximal entry
    onehot = (arg[:, None] == np.arange(D)[None, :]).astype(F64)
    cnt = onehot.sum(0)[:, None]
    dec = float(F32(decay))
    one_m = float(F32(1) - F32(decay))
    with np.errstate(divide="ignore", invalid="ignore"):
        bm = np.where(cnt > 0, (onehot.T @ x64) / cnt, np.nan)
        dev = x64 - np.where(np.isnan(bm), 0.0, bm)[arg]
        bv = np.where(cnt > 1, (onehot.T @ (dev * dev)) / (cnt - 1), np.nan)
    pm, pv = pop_mean.astype(F64), pop_var.astype(F64)
    return (pm * dec + bm * one_m, np.abs(pm * dec) + np.abs(bm * one_m),
            pv * dec + bv * one_m, np.abs(pv * dec) + np.abs(bv * one_m))


def ref64_domain_bn_eval(x, mask, pop_mean, pop_var, eps):
    """out[b] = sum_d mask[b, d] (x[b] - pop_mean[d]) / sqrt(pop_var[d] + eps) (utils.py:626-635).  Returns y, sumabs."""
    x64, m64 = x.astype(F64), mask.astype(F64)
    term = (x64[:, None, :] - pop_mean.astype(F64)[None]) / np.sqrt(pop_var.astype(F64) + float(F32(eps)))[None]
    prod = m64[:, :, None] * term
    return prod.sum(1), np.abs(prod).sum(1)


def model32_domain_bn_update(x, mask, pop_mean, pop_var, decay, mutate=None):
    """statistics in double and one cast (as the kernel's Welford pass), the blend in float32"""
    D = mask.shape[1]
    if mutate == "last_max_wins":
        arg = D - 1 - np.argmax(mask[:, ::-1], axis=1)
    else:
        arg = np.argmax(mask, axis=1)
    nan = F32(np.nan)
    bm, bv = np.zeros_like(pop_mean), np.zeros_like(pop_var)
    for d in range(D):
        xs = x[arg == d].astype(F64)
        c = len(xs)
        bm[d] = xs.mean(0).astype(F32) if c > 0 else (F32(0) if mutate == "empty_gives_zero" else nan)
        if c > 1:
            bv[d] = (((xs - xs.mean(0)) ** 2).sum(0) / (c if mutate == "biased_variance" else c - 1)).astype(F32)
        elif c == 1:
            bv[d] = F32(0) if mutate == "single_variance_zero" else nan
        else:
            bv[d] = F32(0) if mutate == "empty_gives_zero" else nan
    dec = F32(decay)
    return ((pop_mean * dec + bm * (F32(1) - dec)).astype(F32), (pop_var * dec + bv * (F32(1) - dec)).astype(F32))


def model32_domain_bn_eval(x, mask, pop_mean, pop_var, eps, mutate=None):
    e = F32(eps)
    den = (np.sqrt(pop_var) + e).astype(F32) if mutate == "eps_outside_sqrt" else np.sqrt(pop_var + e).astype(F32)
    if mutate == "argmax_eval":
        arg = np.argmax(mask, axis=1)
        return ((x - pop_mean[arg]) / den[arg]).astype(F32)
    acc = np.zeros_like(x)
    for d in range(mask.shape[1]):
        acc = (acc + mask[:, d:d + 1] * ((x - pop_mean[d]) / den[d])).astype(F32)
    return acc


# ---------------------------------------------------------------------------------------------------------------
# the parametrisations both test files share (the GPU file runs them, the CPU file proves them sensitive)
# ---------------------------------------------------------------------------------------------------------------
TWO24 = 2.0 ** -24
APG_FWD_CASES = [(1, 1, 1, 3), (257, 5, 7, 48), (64, 32, 16, 560), (11000, 5, 7, 48)]  # (B, k, E, Kf)
APG_BWD_CASES = [(1, 1, 1), (257, 5, 7), (64, 32, 16), (16385, 32, 3)]                  # (B, k, E)
APG_W_CASES = [(1, 1), (5, 7), (32, 16), (33, 3)]                                        # (k, E)
APG_W_FLAGS = [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
SNR_CASES = [(1, 1, 1, 1), (6, 16, 16, 1), (12, 10, 30, 1), (4, 3, 5, 1),               # (n_blocks, rows, cols, zw)
             (6, 16, 16, 16), (5, 7, 33, 33), (4, 3, 260, 260)]
SNR_ALPHAS = [1.0, 0.05, 7.0]
ES_B = [1, 63, 64, 65, 1024, 1025, 3001]
ES_MODES = ["inference", "autograd", "fused", "loss_only", "draw_only"]
ESCM_WEIGHTS = [(0.1, 1.0), (0.7, 0.3)]
DBN_UPDATE_CASES = [(64, 16, 2, False), (515, 300, 3, False), (7, 5, 4, True)]           # (B, n, D, degenerate)
DBN_DECAYS = [0.9, 0.0]
DBN_EVAL_CASES = [(300, 16, 2), (4099, 130, 3)]
DBN_EPS = 1e-5
TOL_ES, TOL_SNR_W, TOL_SNR_G = 2e-5, 1e-5, 2e-5
TOL_DBN_UPDATE, TOL_DBN_EVAL = 1e-6, 1e-5


def escm_npos_list(B):
    return sorted({min(n, B) for n in (0, 2, 40, int(0.3 * B))})


def esmm_npos(B):
    return max(1, int(0.3 * B))


def es_mode_args(mode):
    """(labels?, dout?, draw?, loss?) of a pointer combination"""
    return dict(inference=(False, False, False, False), autograd=(False, True, True, False),
                fused=(True, False, True, True), loss_only=(True, False, False, True),
                draw_only=(True, False, True, False))[mode]
