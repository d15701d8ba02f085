"""Host-side proof of tests/model_kernel_refs.py, without a GPU:
  * every ref64_* agrees with an independent computation (torch float64 autograd, per-sample / per-domain loops, the oracle);
  * the unmutated float32 restatement model32_* stays inside every tolerance the GPU file uses, at every shape it uses --
    the reference arithmetic alone does not eat the tolerance;
  * every named mutation of model32_* is rejected by assert_close_terms (or by the bit comparison where the GPU file asks
    for bit equality) at every parametrised case where it can apply; the cases where it cannot are named here;
  * the branch census of the input builders is asserted."""
import numpy as np
import pytest
import torch

import model_kernel_refs as R
from model_kernel_refs import F32, F64, assert_close_terms, bits_equal
from oracle import mmlrec_oracle as orc

SENT = F32(np.nan)


def rejected(fn):
    """True if the comparison inside fn() fails"""
    try:
        fn()
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------
# the comparator itself
# ---------------------------------------------------------------------------------------------------------------
def test_comparator_is_elementwise_and_strict_about_nan():
    ref = np.array([1e12, 1.0, 0.0, np.nan])
    sa = np.array([1e12, 1.0, 0.0, np.nan])
    assert assert_close_terms(ref.copy(), ref, sa, 1e-5, "t") == 0.0
    # an error that a max-norm over the 1e12 row would hide
    with pytest.raises(AssertionError, match=r"worst err / \(tol \* sumabs\) = 100 at \(1,\)"):
        assert_close_terms(np.array([1e12, 1.001, 0.0, np.nan]), ref, sa, 1e-5, "t")
    with pytest.raises(AssertionError, match="NaN positions differ"):
        assert_close_terms(np.array([1e12, 1.0, 0.0, 0.0]), ref, sa, 1e-5, "t")
    with pytest.raises(AssertionError, match="NaN positions differ"):
        assert_close_terms(np.array([1e12, np.nan, 0.0, np.nan]), ref, sa, 1e-5, "t")
    with pytest.raises(AssertionError, match="inf"):  # any error over a zero bound
        assert_close_terms(np.array([1e12, 1.0, 1e-30, np.nan]), ref, sa, 1e-5, "t")
    assert abs(assert_close_terms(np.array([1.0 + 5e-6]), np.array([1.0]), np.array([1.0]), 1e-5, "t") - 0.5) < 1e-6


# ---------------------------------------------------------------------------------------------------------------
# APG
# ---------------------------------------------------------------------------------------------------------------
def _apg_torch(o1, s, Wkk, bkk, Wb, do2):
    t = [torch.tensor(a.astype(F64), requires_grad=True) for a in (o1, Wkk, bkk, Wb)]
    o1_, Wkk_, bkk_, Wb_ = t
    s_ = torch.tensor(s.astype(F64))
    k = o1.shape[1]
    Wgen = (s_ @ Wkk_.T + bkk_).view(-1, k, k)                      # apg.py:78-79
    o2 = torch.matmul(o1_.unsqueeze(1), Wgen).squeeze(1) + s_ @ Wb_.T  # apg.py:80, :101
    o2.backward(torch.tensor(do2.astype(F64)))
    return o2.detach().numpy(), [a.grad.numpy() for a in t]


@pytest.mark.parametrize("B,k,E", [(1, 1, 1), (9, 5, 7), (4, 32, 16), (6, 33, 3)])
def test_apg_refs_against_the_generated_weight_form(B, k, E):
    """z @ W_cat is the per-sample generated-weight product, and the features-bwd / unpack references are its autograd."""
    inp, _ = R.build_apg(B, k, E, seed=k * 100 + E)
    w, _ = R.build_apg_weights(k, E, seed=k * 100 + E + 1)
    rng = np.random.default_rng(5)
    do2 = rng.standard_normal((B, k)).astype(F32)
    o2_t, (do1_t, dWkk_t, dbkk_t, dWb_t) = _apg_torch(inp["o1"], inp["s"], w["Wkk"], w["bkk"], w["Wb"], do2)
    Kf = k * E + k + E + 2
    z = R.ref64_apg_features_fwd(inp["o1"], inp["s"], Kf)
    assert (z[:, k * E + k + E:] == 0).all()
    Wc = np.zeros((Kf, k))
    Wc[:k * E + k + E] = R.ref64_apg_pack(w["Wkk"], w["bkk"], w["Wb"], k, E)
    o2, sa = R.ref64_apg_generated(inp["o1"], inp["s"], w["Wkk"], w["bkk"], w["Wb"])
    assert_close_terms(o2, o2_t, sa, 1e-13, "apg generated vs torch")
    assert_close_terms(z @ Wc, o2_t, sa, 1e-13, "apg z @ Wcat vs torch")
    # backward: dz = do2 @ Wcat^T, dWcat = z^T do2
    dz = (do2.astype(F64) @ Wc.T)[:, :k * E + k]
    do1, sa1 = R.ref64_apg_features_bwd(dz, inp["s"], k)  # (float64 dz: astype is a no-op)
    assert_close_terms(do1, do1_t, np.maximum(sa1, 1e-300), 1e-12, "apg do1 vs torch")
    dWcat = (z.T @ do2.astype(F64))[:k * E + k + E]
    (dWkk, _), (dbkk, _), (dWb, _) = R.ref64_apg_unpack(dWcat, k, E)
    for got, ref, nm in ((dWkk, dWkk_t, "dWkk"), (dbkk, dbkk_t, "dbkk"), (dWb, dWb_t, "dWb")):
        assert_close_terms(got, ref, np.abs(ref) + 1e-9, 1e-12, "apg " + nm + " vs torch")


@pytest.mark.parametrize("B,k,E,Kf", R.APG_FWD_CASES)
def test_apg_features_fwd_model_and_mutations(B, k, E, Kf):
    inp, _ = R.build_apg(B, k, E, seed=B + k)
    ref = R.ref64_apg_features_fwd(inp["o1"], inp["s"], Kf).astype(F32)
    prior = np.full((B, Kf), SENT, F32)
    assert bits_equal(R.model32_apg_features_fwd(inp["o1"], inp["s"], Kf, prior), ref)
    # swap_o1_s cannot apply at k = E = 1 (o1[0] s[0] either way); pad_unwritten needs Kf > kE + k + E
    if (k, E) != (1, 1):
        assert not bits_equal(R.model32_apg_features_fwd(inp["o1"], inp["s"], Kf, prior, "swap_o1_s"), ref)
    if Kf > k * E + k + E:
        assert not bits_equal(R.model32_apg_features_fwd(inp["o1"], inp["s"], Kf, prior, "pad_unwritten"), ref)
    else:
        assert (B, k, E, Kf) in ((1, 1, 1, 3), (64, 32, 16, 560))  # Kf exactly kE + k + E: no pad column


@pytest.mark.parametrize("B,k,E,Kf", R.APG_FWD_CASES[:3])
def test_apg_composition_model_and_mutations(B, k, E, Kf):
    """float32 features @ float32 W_cat (product in float64) against the generated-weight form within 2^-23 sum|terms|;
    a transposed feature map or weight map is outside it."""
    inp, _ = R.build_apg(B, k, E, seed=B + k)
    w, _ = R.build_apg_weights(k, E, seed=k + E)
    ref, sa = R.ref64_apg_generated(inp["o1"], inp["s"], w["Wkk"], w["bkk"], w["Wb"])
    prior = np.zeros((B, Kf), F32)

    def run(mz=None, mw=None):
        z = R.model32_apg_features_fwd(inp["o1"], inp["s"], Kf, prior, mz).astype(F64)
        Wc = R.model32_apg_pack(w["Wkk"], w["bkk"], w["Wb"], k, E, mw).astype(F64)
        assert_close_terms(z[:, :k * E + k + E] @ Wc, ref, sa, 2.0 ** -23, "apg composition")
    run()
    if (k, E) != (1, 1):  # (every map is the identity at k = E = 1)
        for mz, mw in (("swap_o1_s", None), (None, "wkk_ji"), (None, "bkk_T"), (None, "wb_Ek")):
            assert rejected(lambda: run(mz, mw)), (mz, mw)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("B,k,E", R.APG_BWD_CASES)
def test_apg_features_bwd_model_and_mutations(B, k, E, accumulate):
    inp, _ = R.build_apg(B, k, E, seed=B + k)
    ref, sa = R.ref64_apg_features_bwd(inp["dz"], inp["s"], k, inp["prior"] if accumulate else None)
    tol = (E + 3) * R.TWO24
    args = (inp["dz"], inp["s"], k, inp["prior"], accumulate)
    assert_close_terms(R.model32_apg_features_bwd(*args), ref, sa, tol, "apg_features_bwd model32")
    muts = ["drop_dz_tail", "E_minus_1"] + (["ignore_accumulate"] if accumulate else [])  # (the flag matters only when set)
    for m in muts:
        assert rejected(lambda: assert_close_terms(R.model32_apg_features_bwd(*args, mutate=m), ref, sa, tol, m)), m


@pytest.mark.parametrize("k,E", R.APG_W_CASES)
def test_apg_weights_model_and_mutations(k, E):
    w, _ = R.build_apg_weights(k, E, seed=k + E)
    ref = R.ref64_apg_pack(w["Wkk"], w["bkk"], w["Wb"], k, E).astype(F32)
    assert bits_equal(R.model32_apg_pack(w["Wkk"], w["bkk"], w["Wb"], k, E), ref)
    # at k = 1 the two transpositions are the identity; Wb [k, E] read as [E, k] is the same memory when k = 1 or E = 1
    layout = [m for m, ok in (("wkk_ji", k > 1), ("bkk_T", k > 1), ("wb_Ek", k > 1 and E > 1)) if ok]
    assert layout or (k, E) == (1, 1)
    for m in layout:
        assert not bits_equal(R.model32_apg_pack(w["Wkk"], w["bkk"], w["Wb"], k, E, m), ref), m
    priors = (w["pWkk"], w["pbkk"], w["pWb"])
    for flags in R.APG_W_FLAGS:
        refs = [v.astype(F32) for v, _ in R.ref64_apg_unpack(w["dWcat"], k, E,
                                                            [p if f else None for p, f in zip(priors, flags)])]
        got = R.model32_apg_unpack(w["dWcat"], k, E, priors, flags)
        assert all(bits_equal(g, r) for g, r in zip(got, refs)), flags
        muts = layout + ["ignore_acc_" + n for n, f in zip(("kk", "bkk", "wb"), flags) if f]
        for m in muts:
            got = R.model32_apg_unpack(w["dWcat"], k, E, priors, flags, m)
            assert not all(bits_equal(g, r) for g, r in zip(got, refs)), (m, flags)


# ---------------------------------------------------------------------------------------------------------------
# SNR
# ---------------------------------------------------------------------------------------------------------------
def _snr_torch(u, alpha, dW, M, zw):
    """autograd through the reference's formula (snr_trans.py:40-43 / mssm.py:42-51)"""
    nb, rows, cols = M.shape
    u_ = torch.tensor(u.astype(F64), requires_grad=True)
    a_ = torch.tensor(alpha.astype(F64), requires_grad=True)
    beta, gamma, eps = (float(F32(c)) for c in (R.SNR_BETA, R.SNR_GAMMA, R.SNR_EPS))
    s = torch.sigmoid(torch.log(u_) - torch.log(1 - u_) + torch.log(a_) / beta)
    s_ = s * (eps - gamma) + gamma
    z = (s_ > 0).double() * s_
    z = (z > 1).double() + (z <= 1).double() * z
    W = z.view(nb, 1, zw) * torch.tensor(M.astype(F64))
    W.backward(torch.tensor(dW.astype(F64)))
    return z.detach().numpy(), u_.grad.numpy(), a_.grad.numpy()


@pytest.mark.parametrize("alpha", R.SNR_ALPHAS)
@pytest.mark.parametrize("nb,rows,cols,zw", R.SNR_CASES)
def test_snr_refs_against_torch_autograd_and_the_oracle(nb, rows, cols, zw, alpha):
    inp, census = R.build_snr(nb, rows, cols, zw, alpha, seed=nb * 1000 + cols)
    z, dzu, dza, sb = R.ref64_snr_z(inp["u"], alpha)
    assert not ((np.abs(sb) < 1e-3) | (np.abs(sb - 1) < 1e-3)).any()  # the branch-distance condition
    zt, du_t, da_t = _snr_torch(inp["u"], inp["alpha"], inp["dW"], inp["M"], zw)
    assert np.abs(z - zt).max() <= 1e-15
    du, du_sa, da, da_sa = R.ref64_snr_bwd(inp["dW"], inp["M"], inp["u"], inp["alpha"], zw)
    live = (sb > 0) & (sb <= 1)
    assert_close_terms(du[live], du_t[live], du_sa[live], 1e-12, "snr du vs torch")
    assert (du[~live] == 0).all() and (du_t[~live] == 0).all() and (du_sa[~live] == 0).all()  # saturated: exact zeros
    assert set(np.unique(z[~live])) <= {0.0, 1.0}
    assert_close_terms(da, da_t, np.maximum(da_sa, 1e-300), 1e-12, "snr dalpha vs torch")
    zo, dzu_o, dza_o = orc.snr_z(inp["u"], inp["alpha"])
    # (the oracle reads beta / gamma / eps as float64 literals, the reference at their float32 values: z = s 1.2 - 0.1 is
    # judged against its two terms)
    assert_close_terms(zo, z, np.abs(sb - R.SNR_GAMMA) + abs(R.SNR_GAMMA), 1e-6, "snr z vs oracle")
    assert_close_terms(dzu_o, dzu, np.abs(dzu), 1e-6, "snr dz/du vs oracle")
    assert_close_terms(dza_o, dza, np.abs(dza), 1e-6, "snr dz/dalpha vs oracle")


def test_snr_census():
    """alpha 1.0: some coefficients dead, some at one; alpha 7.0: many at one; 0.05: many dead -- on the uniform fill."""
    for alpha, lo_dead, lo_one in ((1.0, 0.05, 0.05), (7.0, 0.0, 0.35), (0.05, 0.35, 0.0)):
        _, c = R.build_snr(40, 2, 100, 100, alpha, seed=5)
        assert c["dead"] >= lo_dead * c["n"] and c["one"] >= lo_one * c["n"] and c["live"] > 0.2 * c["n"], (alpha, c)
    for case in R.SNR_CASES:  # every case larger than one coefficient has all three regimes at alpha 1.0
        _, c = R.build_snr(*case, 1.0, seed=case[0] * 1000 + case[2])
        assert c["n"] == 1 or (c["dead"] and c["one"] and c["live"]), (case, c)


@pytest.mark.parametrize("alpha", R.SNR_ALPHAS)
@pytest.mark.parametrize("nb,rows,cols,zw", R.SNR_CASES)
def test_snr_model_and_mutations(nb, rows, cols, zw, alpha):
    inp, census = R.build_snr(nb, rows, cols, zw, alpha, seed=nb * 1000 + cols)
    u, al, M, dW = inp["u"], inp["alpha"], inp["M"], inp["dW"]
    W, Wsa, zexp = R.ref64_snr_fwd(u, al, M, zw)
    got = R.model32_snr_fwd(u, al, M, zw)
    assert_close_terms(got, W, Wsa, R.TOL_SNR_W, "snr_fwd model32")
    sat0, sat1 = zexp == 0.0, zexp == 1.0
    assert bits_equal(got[sat0], (F32(0) * M)[sat0]) and bits_equal(got[sat1], M[sat1])
    _, _, _, sb = R.ref64_snr_z(u, alpha)
    one_single = nb * zw == 1

    def fwd_rejects(m):
        return rejected(lambda: assert_close_terms(R.model32_snr_fwd(u, al, M, zw, m), W, Wsa, R.TOL_SNR_W, m))
    # log(alpha) * beta is log(alpha) / beta at alpha = 1; the single coefficient 0.97 stays at one under both forms at
    # alpha = 7
    if alpha != 1.0 and not (one_single and alpha == 7.0):
        assert fwd_rejects("log_alpha_times_beta")
    if zw > 1:  # (needs more than one column and more than one row, which every zw > 1 case has)
        assert fwd_rejects("zw_col_div")

    for acc_u in (0, 1):
        for acc_a in (0, 1):
            for want_du in ((True, False) if zw > 1 else (True,)):
                du, du_sa, da, da_sa = R.ref64_snr_bwd(dW, M, u, al, zw, inp["prior_du"] if acc_u else None,
                                                       inp["prior_dalpha"] if acc_a else None)

                def check(m=None):
                    gdu, gda = R.model32_snr_bwd(dW, M, u, al, zw, inp["prior_du"], inp["prior_dalpha"], acc_u, acc_a,
                                                 want_du, m)
                    if want_du:
                        assert_close_terms(gdu, du, du_sa, R.TOL_SNR_G, "snr_bwd du " + str(m))
                    assert_close_terms(gda, da, da_sa, R.TOL_SNR_G, "snr_bwd dalpha " + str(m))
                check()
                muts = []
                # a coefficient above one whose sigmoid still has a slope: its du shows it element-wise; its share of
                # the dalpha sum is below the tolerance (s (1 - s) is tiny up there), so the frozen-u call cannot
                if census["one"] and want_du:
                    muts.append("deriv_above_saturation")
                if alpha != 1.0 and census["live"]:
                    muts.append("log_alpha_times_beta")
                # the last block's share of dalpha is zero when all its coefficients are saturated: only (1,1,1) at
                # alpha 1.0 / 7.0, whose one coefficient is at one
                last_live = ((sb > 0) & (sb <= 1)).reshape(nb, -1)[-1].any()
                assert last_live or (one_single and alpha != 0.05)
                if last_live:
                    muts.append("dalpha_misses_last_block")
                if want_du and acc_u:
                    muts.append("acc_u_ignored")
                if want_du and census["live"]:
                    muts.append("du_with_dz_dalpha")
                for m in muts:
                    assert rejected(lambda: check(m)), (m, acc_u, acc_a, want_du)


# ---------------------------------------------------------------------------------------------------------------
# ESMM / ESCM
# ---------------------------------------------------------------------------------------------------------------
def _torch_bce_loss(praw, y, model, cf_w=0.1, global_w=1.0):
    p = torch.tensor(praw.astype(F64), requires_grad=True)
    yt = torch.tensor(y.astype(F64))
    bce = torch.nn.functional.binary_cross_entropy
    c, v = p[:, 0], p[:, 1]
    if model == "esmm":
        loss = bce(c, yt[:, 0], reduction="sum") + bce(c * v, yt[:, 1], reduction="sum")
    else:  # the form tests/test_models_gpu.py uses for ESCM
        n_ctr = yt[:, 0].sum()
        ips = torch.clip(1.0 / torch.maximum(c * n_ctr, torch.full_like(c, 1e-6)), -15, 15) * len(yt)
        ipw = (bce(v, yt[:, 1], reduction="sum") * ips * yt[:, 0]).mean()
        loss = bce(c, yt[:, 0], reduction="sum") + float(F32(cf_w)) * ipw \
            + float(F32(global_w)) * bce(c * v, yt[:, 1], reduction="sum")
    loss.backward()
    return float(loss), p.grad.numpy()


ESCM_CASES = [(B, npos, w) for B in R.ES_B for npos in R.escm_npos_list(B) for w in R.ESCM_WEIGHTS]


@pytest.mark.parametrize("B", R.ES_B)
def test_esmm_ref_against_torch_autograd(B):
    inp, _ = R.build_escm(B, R.esmm_npos(B))
    r = R.ref64_esmm(inp["praw"], inp["y"])
    tl, tg = _torch_bce_loss(inp["praw"], inp["y"], "esmm")
    assert abs(r["loss"] - tl) <= 1e-12 * tl
    # (the residue is torch's float32 constant 1e-12 against the float64 literal: rows on the floor only)
    assert_close_terms(r["draw"], tg, r["draw_sumabs"], 1e-8, "esmm draw vs torch")
    a = R.ref64_esmm(inp["praw"], None, inp["dout2"])
    d, c, v = inp["dout2"].astype(F64), inp["praw"][:, 0].astype(F64), inp["praw"][:, 1].astype(F64)
    assert np.array_equal(a["draw"], np.stack([d[:, 0] + d[:, 1] * v, d[:, 1] * c], 1))


@pytest.mark.parametrize("B,npos,w", ESCM_CASES)
def test_escm_ref_against_torch_autograd_and_the_oracle(B, npos, w):
    inp, census = R.build_escm(B, npos)
    assert not R.escm_near_threshold(inp["praw"][:, 0], inp["praw"][:, 1], inp["y"][:, 0]).any()
    r = R.ref64_escm(inp["praw"], inp["y"], None, *w)
    tl, tg = _torch_bce_loss(inp["praw"], inp["y"], "escm", *w)
    assert abs(r["loss"] - tl) <= 1e-12 * abs(tl)
    assert_close_terms(r["draw"], tg, r["draw_sumabs"], 1e-8, "escm draw vs torch")
    # the oracle at its float32 precision (it returns the direct terms; the product's chain rule is applied here)
    c, v = inp["praw"][:, 0], inp["praw"][:, 1]
    ol, od = orc.escm_loss_and_dprob(np.stack([c, v, c * v], 1), inp["y"], float(F32(w[0])), float(F32(w[1])))
    assert abs(ol - r["loss"]) <= 2e-5 * r["loss"]
    od = od.astype(F64)
    chain = np.stack([od[:, 0] + od[:, 2] * v, od[:, 1] + od[:, 2] * c], 1)
    assert_close_terms(chain, r["draw"], r["draw_sumabs"], 2e-5, "escm draw vs oracle")


def test_escm_census_covers_the_three_ipw_regimes():
    for B, npos in ((1024, 40), (3001, 40), (3001, 900)):
        _, c = R.build_escm(B, npos)
        assert c["unclipped"] >= 1 and c["clipped"] >= 1 and c["floored"] >= 1, (B, npos, c)
        assert c["unclipped"] + c["clipped"] + c["floored"] == npos
    for B in (1025, 3001):  # the rows behind the first 1024 hold positives whenever the case has at least 40
        assert R.build_escm(B, 40)[1]["pos_beyond_1024"] >= (1 if B == 3001 else 0)


def _es_compare(got, ref, what, loss_tol=R.TOL_ES):
    assert bits_equal(got["pout"], ref["pout"].astype(F32)), what + ": p_out"
    if ref["loss"] is not None and got["loss"] is not None:
        assert_close_terms(np.array([got["loss"]]), np.array([ref["loss"]]), np.array([abs(ref["loss"])]), loss_tol,
                           what + ": loss")
    if got["draw"] is not None:
        assert_close_terms(got["draw"], ref["draw"], ref["draw_sumabs"], R.TOL_ES, what + ": draw")


@pytest.mark.parametrize("mode", R.ES_MODES)
@pytest.mark.parametrize("B", R.ES_B)
def test_esmm_model_and_mutations(B, mode):
    has_y, has_dout, has_draw, has_loss = R.es_mode_args(mode)
    inp, _ = R.build_escm(B, R.esmm_npos(B))
    y, dout = (inp["y"] if has_y else None), (inp["dout2"] if has_dout else None)
    ref = R.ref64_esmm(inp["praw"], y, dout)

    def run(m=None):
        _es_compare(R.model32_esmm(inp["praw"], y, dout, has_draw, has_loss, mutate=m), ref, "esmm " + str(m))
    run()
    muts = []
    # B <= 64 (1, 63, 64): wave 0 holds every row; B = 65: the one row behind wave 0 adds less than 2e-5 of a loss
    # that holds the saturated rows' clamped 100s
    if has_loss and B > 65:
        muts.append("wave0_only")
    if B > 1024:                  # (1025, 3001)
        muts.append("skip_rows_ge_1024")
    if B == 1:  # the single row's cvr is 6e-9-ish: under the autograd path's unit-sized g0 the g1 v term is below 2e-5
        assert inp["praw"][0, 1] < 1e-5
    if has_draw and not (B == 1 and mode == "autograd"):
        muts.append("dctr_without_g1v")
    if has_loss and B >= 4:       # B = 1 has no saturated row (the first B // 4 rows), so no log term reaches -100
        muts.append("loss_without_clamp")
    for m in muts:
        assert rejected(lambda: run(m)), m


@pytest.mark.parametrize("mode", R.ES_MODES)
@pytest.mark.parametrize("B,npos,w", ESCM_CASES)
def test_escm_model_and_mutations(B, npos, w, mode):
    has_y, has_dout, has_draw, has_loss = R.es_mode_args(mode)
    inp, census = R.build_escm(B, npos)
    y, dout = (inp["y"] if has_y else None), (inp["dout3"] if has_dout else None)
    ref = R.ref64_escm(inp["praw"], y, dout, *w)

    def run(m=None):
        _es_compare(R.model32_escm(inp["praw"], y, dout, *w, has_draw, has_loss, mutate=m), ref, "escm " + str(m))
    run()
    if not has_y:
        return  # (the label-free paths have no branch to mutate; their arithmetic is the comparison above)
    y1 = inp["y"][:, 1]
    L1 = R._bce64(inp["praw"][:, 1].astype(F64), y1.astype(F64)).sum()
    muts = []
    # the IPW derivative outside its regime: needs a positive row that is clipped or floored, and a draw output
    if has_draw and census["clipped"] + census["floored"] > 0 and L1 > 0:
        muts.append("dips_when_clipped")
    # S over all rows: needs rows with y0 = 0 (every case but B = npos = 1), and L1 > 0 for the loss / N > 0 ... S also
    # scales d/d cvr, so either output shows it
    if census["neg"] > 0 and L1 > 0:
        muts.append("S_without_y0")
    # N over the first 1024 rows: needs positives behind them (B = 1025 holds one only by chance: census decides)
    if census["pos_beyond_1024"] > 0 and census["N"] > 0:
        muts.append("N_first_1024_rows")
    if has_draw and census["N"] > 0:  # S = 0 without positives: the term vanishes
        muts.append("draw1_without_cf_S_g1")
    if has_draw and w[1] != 1.0:      # global_w = 1.0 multiplies by one
        muts.append("g2_without_global_w")
    muts.append("cf_w_on_L0")
    for m in muts:
        assert rejected(lambda: run(m)), (m, census)


def test_escm_mutations_apply_where_the_issue_needs_them():
    """The census-driven applicability above must not be vacuous: at the three large cases every ESCM mutation applies in
    the fused mode (global_w needs the second weight pair)."""
    for B, npos in ((1024, 40), (3001, 40), (3001, 900)):
        _, c = R.build_escm(B, npos)
        assert c["clipped"] + c["floored"] > 0 and c["neg"] > 0 and c["N"] > 0
        assert c["pos_beyond_1024"] > 0 or B == 1024


# ---------------------------------------------------------------------------------------------------------------
# DomainBN
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", R.DBN_DECAYS)
@pytest.mark.parametrize("B,n,D,degenerate", R.DBN_UPDATE_CASES)
def test_domain_bn_update_ref_model_and_mutations(B, n, D, degenerate, decay):
    inp, census = R.build_domain_bn(B, n, D, seed=B + n, degenerate=degenerate)
    x, mask, pm, pv = inp["x"], inp["mask"], inp["pop_mean"], inp["pop_var"]
    assert census["tie_first"] == (0 if degenerate else D - 2)
    assert (census["empty"], census["single"]) == ((1, 1) if degenerate else (0, 0))
    m, m_sa, v, v_sa = R.ref64_domain_bn_update(x, mask, pm, pv, decay)
    # independent: the per-domain loop of utils.py:582-584 in torch float64 (mean / var of an empty selection: NaN)
    dom = torch.argmax(torch.tensor(mask), dim=1)
    xt = torch.tensor(x.astype(F64))
    dec, one_m = float(F32(decay)), float(F32(1) - F32(decay))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for d in range(D):
            sel = xt[dom == d]
            bm, bv = sel.mean(0).numpy(), sel.var(0, unbiased=True).numpy()
            assert_close_terms(m[d], pm[d].astype(F64) * dec + bm * one_m, m_sa[d], 1e-13, "dbn mean vs loop")
            assert_close_terms(v[d], pv[d].astype(F64) * dec + bv * one_m, v_sa[d], 1e-12, "dbn var vs loop")
    if degenerate:
        assert np.isnan(m[D - 1]).all() and np.isnan(v[D - 1]).all()          # the empty domain
        assert np.isfinite(m[D - 2]).all() and np.isnan(v[D - 2]).all()       # the one-sample domain
        assert np.isfinite(m[:D - 2]).all() and np.isfinite(v[:D - 2]).all()

    def run(mut=None):
        gm, gv = R.model32_domain_bn_update(x, mask, pm, pv, decay, mut)
        assert_close_terms(gm, m, m_sa, R.TOL_DBN_UPDATE, "dbn_update mean " + str(mut))
        assert_close_terms(gv, v, v_sa, R.TOL_DBN_UPDATE, "dbn_update var " + str(mut))
    run()
    muts = ["biased_variance", "last_max_wins"]
    if degenerate:  # only (7, 5, 4) has an empty and a one-sample domain
        muts += ["empty_gives_zero", "single_variance_zero"]
    for mut in muts:
        assert rejected(lambda: run(mut)), mut


@pytest.mark.parametrize("B,n,D", R.DBN_EVAL_CASES)
def test_domain_bn_eval_ref_model_and_mutations(B, n, D):
    inp, census = R.build_domain_bn(B, n, D, seed=B + n, soft=True)
    x, mask, pm, pv = inp["x"], inp["mask"], inp["pop_mean"], inp["pop_var"]
    assert len(census["soft_rows"]) == 3 and (mask[census["zero_row"]] == 0).all()
    y, sa = R.ref64_domain_bn_eval(x, mask, pm, pv, R.DBN_EPS)
    # independent: F.batch_norm per domain in eval mode, weighted by the mask (utils.py:626-635)
    xt = torch.tensor(x.astype(F64))
    outs = [torch.nn.functional.batch_norm(xt, torch.tensor(pm[d].astype(F64)), torch.tensor(pv[d].astype(F64)),
                                           eps=float(F32(R.DBN_EPS))) for d in range(D)]
    yt = (torch.tensor(mask.astype(F64)).unsqueeze(-1) * torch.stack(outs, 1)).sum(1).numpy()
    # (F.batch_norm may scale before it subtracts: judged against |x| + |pop_mean|, not against the difference)
    sa_t = (np.abs(mask.astype(F64))[:, :, None] * (np.abs(x.astype(F64))[:, None, :] + np.abs(pm.astype(F64))[None])
            / np.sqrt(pv.astype(F64) + float(F32(R.DBN_EPS)))[None]).sum(1)
    assert_close_terms(y, yt, np.maximum(sa_t, 1e-300), 1e-13, "dbn eval vs torch")
    assert (y[census["zero_row"]] == 0).all()

    def run(mut=None):
        assert_close_terms(R.model32_domain_bn_eval(x, mask, pm, pv, R.DBN_EPS, mut), y, sa, R.TOL_DBN_EVAL,
                           "dbn_eval " + str(mut))
    run()
    for mut in ("argmax_eval", "eps_outside_sqrt"):
        assert rejected(lambda: run(mut)), mut
    # a NaN domain poisons every row (0 * NaN)
    pm2 = pm.copy()
    pm2[D - 1] = np.nan
    assert np.isnan(R.ref64_domain_bn_eval(x, mask, pm2, pv, R.DBN_EPS)[0]).all()
