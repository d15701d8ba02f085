"""Kernel-level parity of the nine C-ABI entry points of csrc/apg.hip, csrc/snr.hip, csrc/esmm.hip and the domain part
of csrc/bn.hip against the float64 references of tests/model_kernel_refs.py (proved on the host by
tests/test_model_kernel_refs_cpu.py).  Every call goes through _lib.load() with raw pointers; every output buffer,
its leading-dimension padding and one row behind it are pre-filled with a NaN sentinel, the written elements are
compared element by element against tol * sum|terms| (never in max-norm) and the padding must keep the sentinel's bits.

Worst observed err / (tol * sum|terms|) per entry point on an MI355X (first device run; printed again at the end of
every run with -s).  The bit-equality checks (features fwd, weights, p_out, saturated SNR blocks) have no ratio.
  mml_apg_features_bwd       0.505   (16385, 32, 3) with accumulate: 3 fma + the prior's add = 4 roundings against a
                                     bound of E + 3 = 6; the worst of 524 320 elements reaches 3 of them (a float64
                                     emulation of the fma chain on the host gives the same 0.505)
  z @ W_cat (composition)    0.162
  mml_snr_gate_weights_fwd   0.022
  mml_snr_gate_weights_bwd   0.039
  mml_esmm_combine           0.253   (the float32 rounding of ctr * cvr under 1 / (1 - p); float32 numpy gives the same)
  mml_escm_combine           0.020
  mml_domain_bn_update       0.118
  mml_domain_bn_eval         0.018
No case failed; no kernel was changed.  Sensitivity on the device (once, while writing this file): a library built
with five in-bounds mutations -- ESMM loss from wave 0's partial only, ESCM's IPW derivative applied when clipped, the SNR
column taken as i / zw, `>=` in DomainBN's arg-max, bkk packed transposed -- failed exactly the tests that cover them
(test_esmm_combine at B >= 1024, test_escm_combine wherever a positive is clipped, test_snr_gate_weights_fwd at zw > 1,
test_domain_bn_update, test_apg_weights / test_apg_composition at k > 1) and no other.
"""
import numpy as np
import pytest
import torch

import model_kernel_refs as R
from model_kernel_refs import F32, F64, assert_close_terms, bits_equal

pytestmark = pytest.mark.gpu

SENT_BITS = np.uint32(0x7FC5A5A5)  # a quiet NaN with a payload no arithmetic produces


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L
    R.RATIOS.clear()
    yield L.load()
    print("\nworst err / (tol * sum|terms|):")
    for k in sorted(R.RATIOS):
        print(f"  {k:32s} {R.RATIOS[k]:.3f}")


def stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """A [rows, cols] float32 matrix inside a [rows + 1, ld] device buffer whose every other element is the sentinel."""

    def __init__(self, rows, cols, ld=None, data=None):
        self.rows, self.cols, self.ld = rows, cols, cols if ld is None else ld
        host = np.full((rows + 1, self.ld), SENT_BITS, np.uint32)
        if data is not None:
            host[:rows, :cols] = np.ascontiguousarray(data, dtype=F32).reshape(rows, cols).view(np.uint32)
        self.t = torch.from_numpy(host.view(F32)).to(dev())

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self, what):
        """the written region; the padding columns and the row behind must still hold the sentinel's bits"""
        host = self.t.cpu().numpy().view(np.uint32)
        assert (host[:self.rows, self.cols:] == SENT_BITS).all(), what + ": a padding column was written"
        assert (host[self.rows] == SENT_BITS).all(), what + ": written behind the last row"
        return host[:self.rows, :self.cols].view(F32).copy()


def vec(data, pad=3):
    data = np.asarray(data, dtype=F32).reshape(1, -1)
    return Buf(1, data.shape[1], data.shape[1] + pad, data)


def ptr(b):
    return None if b is None else b.ptr


def ok(lib, rc):
    assert rc == 0, (rc, lib.mml_last_error())


# ---------------------------------------------------------------------------------------------------------------
# APG
# ---------------------------------------------------------------------------------------------------------------
def _apg_pads(B):
    return (3, 2, 4) if B == 257 else (0, 0, 0)  # (ldo1 - k, lds - E, ldz - Kf)


@pytest.mark.parametrize("B,k,E,Kf", R.APG_FWD_CASES)
def test_apg_features_fwd(lib, B, k, E, Kf):
    """Bit-equal to the float32 product; the pad columns [kE + k + E, Kf) are +0.0.  (11000, 5, 7, 48) is the first size
    above 2048 x 256 threads: the grid-stride loop runs twice."""
    inp, _ = R.build_apg(B, k, E, seed=B + k)
    p1, ps, pz = _apg_pads(B)
    o1, s, z = Buf(B, k, k + p1, inp["o1"]), Buf(B, E, E + ps, inp["s"]), Buf(B, Kf, Kf + pz)
    assert (B * Kf > 2048 * 256) == (B == 11000)
    ok(lib, lib.mml_apg_features_fwd(o1.ptr, o1.ld, s.ptr, s.ld, z.ptr, z.ld, B, k, E, Kf, stream()))
    ref = R.ref64_apg_features_fwd(inp["o1"], inp["s"], Kf).astype(F32)
    got = z.get("apg_features_fwd z")
    assert bits_equal(got, ref), np.argwhere(got.view(np.uint32) != ref.view(np.uint32))[:5]
    assert bits_equal(o1.get("o1"), inp["o1"]) and bits_equal(s.get("s"), inp["s"])  # inputs and their padding intact


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("B,k,E", R.APG_BWD_CASES)
def test_apg_features_bwd(lib, B, k, E, accumulate):
    """(E + 3) 2^-24 sum|terms|: E + 1 products, E + 2 additions, fma contraction in either direction.  (16385, 32, 3)
    is the first size above 2048 x 256 threads."""
    inp, _ = R.build_apg(B, k, E, seed=B + k)
    dz, s = Buf(B, k * E + k, k * E + k + 1, inp["dz"]), Buf(B, E, E + 2, inp["s"])
    do1 = Buf(B, k, k + 2, inp["prior"])
    assert (B * k > 2048 * 256) == (B == 16385)
    ok(lib, lib.mml_apg_features_bwd(dz.ptr, dz.ld, s.ptr, s.ld, do1.ptr, do1.ld, B, k, E, accumulate, stream()))
    ref, sa = R.ref64_apg_features_bwd(inp["dz"], inp["s"], k, inp["prior"] if accumulate else None)
    assert_close_terms(do1.get("do1"), ref, sa, (E + 3) * R.TWO24, "mml_apg_features_bwd: do1")


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("k,E", R.APG_W_CASES)
def test_apg_weights(lib, k, E, pad):
    """dir 0: bit-equal to the re-layout; dir 1 over non-zero priors with all flags 0, all 1 and each alone: bit-equal to
    the float32 copy or add."""
    w, c = R.build_apg_weights(k, E, seed=k + E)
    rows = c["rows"]
    Wkk, bkk, Wb = Buf(k * k, E, data=w["Wkk"]), vec(w["bkk"]), Buf(k, E, data=w["Wb"])
    Wcat = Buf(rows, k, k + pad)
    ok(lib, lib.mml_apg_weights(Wkk.ptr, bkk.ptr, Wb.ptr, Wcat.ptr, Wcat.ld, k, E, 0, 0, 0, 0, stream()))
    assert bits_equal(Wcat.get("Wcat"), R.ref64_apg_pack(w["Wkk"], w["bkk"], w["Wb"], k, E).astype(F32))
    assert bits_equal(Wkk.get("Wkk"), w["Wkk"]) and bits_equal(bkk.get("bkk")[0], w["bkk"])
    assert bits_equal(Wb.get("Wb"), w["Wb"])
    priors = (w["pWkk"], w["pbkk"], w["pWb"])
    for flags in R.APG_W_FLAGS:
        dWkk, dbkk, dWb = Buf(k * k, E, data=w["pWkk"]), vec(w["pbkk"]), Buf(k, E, data=w["pWb"])
        dWcat = Buf(rows, k, k + pad, w["dWcat"])
        ok(lib, lib.mml_apg_weights(dWkk.ptr, dbkk.ptr, dWb.ptr, dWcat.ptr, dWcat.ld, k, E, 1, *flags, stream()))
        refs = R.ref64_apg_unpack(w["dWcat"], k, E, [p if f else None for p, f in zip(priors, flags)])
        gots = (dWkk.get("dWkk"), dbkk.get("dbkk")[0], dWb.get("dWb"))
        for got, (ref, _), nm in zip(gots, refs, ("dWkk", "dbkk", "dWb")):
            assert bits_equal(got, ref.astype(F32)), (nm, flags)
        assert bits_equal(dWcat.get("dWcat"), w["dWcat"])


@pytest.mark.parametrize("B,k,E,Kf", R.APG_FWD_CASES[:3])
def test_apg_composition(lib, B, k, E, Kf):
    """z @ W_cat (both downloaded, product in float64) is the per-sample generated-weight formula of the reference:
    within 2^-23 sum|terms| (one float32 rounding per feature product)."""
    inp, _ = R.build_apg(B, k, E, seed=B + k)
    w, c = R.build_apg_weights(k, E, seed=k + E)
    o1, s, z = Buf(B, k, data=inp["o1"]), Buf(B, E, data=inp["s"]), Buf(B, Kf)
    ok(lib, lib.mml_apg_features_fwd(o1.ptr, o1.ld, s.ptr, s.ld, z.ptr, z.ld, B, k, E, Kf, stream()))
    Wkk, bkk, Wb = Buf(k * k, E, data=w["Wkk"]), vec(w["bkk"]), Buf(k, E, data=w["Wb"])
    Wcat = Buf(Kf, k, data=np.zeros((Kf, k), F32))  # (the engine keeps the pad rows of W_cat zero)
    ok(lib, lib.mml_apg_weights(Wkk.ptr, bkk.ptr, Wb.ptr, Wcat.ptr, Wcat.ld, k, E, 0, 0, 0, 0, stream()))
    o2 = z.get("z").astype(F64) @ Wcat.get("Wcat").astype(F64)
    ref, sa = R.ref64_apg_generated(inp["o1"], inp["s"], w["Wkk"], w["bkk"], w["Wb"])
    assert_close_terms(o2, ref, sa, 2.0 ** -23, "apg z @ Wcat: o2")


# ---------------------------------------------------------------------------------------------------------------
# SNR
# ---------------------------------------------------------------------------------------------------------------
def _snr_consts():
    return float(F32(R.SNR_BETA)), float(F32(R.SNR_GAMMA)), float(F32(R.SNR_EPS))


@pytest.mark.parametrize("alpha", R.SNR_ALPHAS)
@pytest.mark.parametrize("nb,rows,cols,zw", R.SNR_CASES)
def test_snr_gate_weights_fwd(lib, nb, rows, cols, zw, alpha):
    """W = z M within 1e-5 |M| element by element; blocks / columns whose coefficient is saturated are bit-equal to 0 M
    (signed zeros) and to M."""
    inp, census = R.build_snr(nb, rows, cols, zw, alpha, seed=nb * 1000 + cols)
    block = rows * cols
    u, al, M, W = vec(inp["u"]), vec(inp["alpha"]), vec(inp["M"]), Buf(1, nb * block, nb * block + 7)
    ok(lib, lib.mml_snr_gate_weights_fwd(u.ptr, al.ptr, M.ptr, W.ptr, nb, block, zw, *_snr_consts(), stream()))
    ref, sa, zexp = R.ref64_snr_fwd(inp["u"], inp["alpha"], inp["M"], zw)
    got = W.get("W").reshape(nb, rows, cols)
    assert_close_terms(got, ref, sa, R.TOL_SNR_W, "mml_snr_gate_weights_fwd: W")
    sat0, sat1 = zexp == 0.0, zexp == 1.0
    assert sat0.sum() == census["dead"] * block // zw and sat1.sum() == census["one"] * block // zw
    assert bits_equal(got[sat0], (F32(0) * inp["M"])[sat0]), "a dead coefficient's block is not 0 * M"
    assert bits_equal(got[sat1], inp["M"][sat1]), "a coefficient at one does not copy M"


@pytest.mark.parametrize("alpha", R.SNR_ALPHAS)
@pytest.mark.parametrize("nb,rows,cols,zw", R.SNR_CASES)
def test_snr_gate_weights_bwd(lib, nb, rows, cols, zw, alpha):
    """du / dalpha within 2e-5 sum|terms| for the four (acc_u, acc_alpha) combinations over non-zero priors, du = NULL
    for zw > 1; a second call on the same inputs gives identical bits (the fixed-order claim of the file header)."""
    inp, census = R.build_snr(nb, rows, cols, zw, alpha, seed=nb * 1000 + cols)
    block = rows * cols
    u, al, M, dW = vec(inp["u"]), vec(inp["alpha"]), vec(inp["M"]), vec(inp["dW"])
    for acc_u in (0, 1):
        for acc_a in (0, 1):
            for want_du in ((True, False) if zw > 1 else (True,)):
                if not want_du and acc_u:
                    continue
                outs = []
                for rep in range(2):
                    du = vec(inp["prior_du"]) if want_du else None
                    da, ws = vec(inp["prior_dalpha"]), Buf(1, nb, nb + 5)
                    ok(lib, lib.mml_snr_gate_weights_bwd(dW.ptr, M.ptr, u.ptr, al.ptr, ptr(du), da.ptr, acc_u, acc_a, nb,
                                                         block, zw, *_snr_consts(), ws.ptr, stream()))
                    ws.get("workspace")  # (nothing behind its n_blocks floats)
                    outs.append((du.get("du")[0] if want_du else None, da.get("dalpha")[0]))
                rdu, rdu_sa, rda, rda_sa = R.ref64_snr_bwd(inp["dW"], inp["M"], inp["u"], inp["alpha"], zw,
                                                           inp["prior_du"] if acc_u else None,
                                                           inp["prior_dalpha"] if acc_a else None)
                if want_du:
                    assert_close_terms(outs[0][0], rdu, rdu_sa, R.TOL_SNR_G, "mml_snr_gate_weights_bwd: du")
                    assert bits_equal(outs[0][0], outs[1][0])
                assert_close_terms(outs[0][1], rda, rda_sa, R.TOL_SNR_G, "mml_snr_gate_weights_bwd: dalpha")
                assert bits_equal(outs[0][1], outs[1][1])


# ---------------------------------------------------------------------------------------------------------------
# ESMM / ESCM
# ---------------------------------------------------------------------------------------------------------------
ES_LDS = {"esmm": [dict(ldr=2, ldy=2, ldo=2, lddo=2, lddr=2), dict(ldr=5, ldy=3, ldo=4, lddo=4, lddr=3)],
          "escm": [dict(ldr=2, ldy=2, ldo=3, lddo=3, lddr=2), dict(ldr=5, ldy=3, ldo=4, lddo=4, lddr=3)]}


def _combine(lib, model, inp, mode, ld, weights=()):
    """one call of mml_esmm_combine / mml_escm_combine -> dict(pout, loss, draw) as downloaded"""
    has_y, has_dout, has_draw, has_loss = R.es_mode_args(mode)
    B = len(inp["praw"])
    nout = 2 if model == "esmm" else 3
    praw = Buf(B, 2, ld["ldr"], inp["praw"])
    y = Buf(B, 2, ld["ldy"], inp["y"]) if has_y else None
    dout = Buf(B, nout, ld["lddo"], inp["dout2" if model == "esmm" else "dout3"]) if has_dout else None
    pout = Buf(B, nout, ld["ldo"])
    draw = Buf(B, 2, ld["lddr"]) if has_draw else None
    loss = Buf(1, 1, 4) if has_loss else None
    fn = lib.mml_esmm_combine if model == "esmm" else lib.mml_escm_combine
    ok(lib, fn(praw.ptr, praw.ld, ptr(y), ld["ldy"], ptr(dout), ld["lddo"], pout.ptr, pout.ld, ptr(draw), ld["lddr"],
               ptr(loss), B, *[float(F32(w)) for w in weights], stream()))
    what = f"mml_{model}_combine"
    return dict(pout=pout.get(what + " p_out"), loss=loss.get(what + " loss")[0, 0] if has_loss else None,
                draw=draw.get(what + " d_raw") if has_draw else None)


def _es_check(got, ref, what):
    assert bits_equal(got["pout"], ref["pout"].astype(F32)), what + ": p_out is not the float32 product"
    if got["loss"] is not None:
        assert_close_terms(np.array([got["loss"]]), np.array([ref["loss"]]), np.array([abs(ref["loss"])]), R.TOL_ES,
                           what + ": loss")
    if got["draw"] is not None:
        assert_close_terms(got["draw"], ref["draw"], ref["draw_sumabs"], R.TOL_ES, what + ": d_raw")


def _es_same_bits(a, b):
    return all((a[k] is None and b[k] is None) or bits_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


@pytest.mark.parametrize("B", R.ES_B)
def test_esmm_combine(lib, B):
    """p_out bit-equal, loss within 2e-5 relative, gradients within 2e-5 sum|terms| element by element (the saturated
    rows' 1e12 hide nothing), for both leading-dimension sets and the five pointer combinations; two calls: same bits."""
    inp, _ = R.build_escm(B, R.esmm_npos(B))
    for ld in ES_LDS["esmm"]:
        for mode in R.ES_MODES:
            has_y, has_dout, _, _ = R.es_mode_args(mode)
            ref = R.ref64_esmm(inp["praw"], inp["y"] if has_y else None, inp["dout2"] if has_dout else None)
            got = _combine(lib, "esmm", inp, mode, ld)
            _es_check(got, ref, "mml_esmm_combine")
            if mode == "fused":
                assert _es_same_bits(got, _combine(lib, "esmm", inp, mode, ld))


ESCM_CASES = [(B, npos) for B in R.ES_B for npos in R.escm_npos_list(B)]


@pytest.mark.parametrize("B,npos", ESCM_CASES)
def test_escm_combine(lib, B, npos):
    """As test_esmm_combine, with npos positives (0: N = 0) and both (cf_w, global_w) pairs; the positives of the larger
    cases cover the floored, clipped and unclipped regimes of the counterfactual-IPW term (census asserted on the host)."""
    inp, _ = R.build_escm(B, npos)
    for w in R.ESCM_WEIGHTS:
        for ld in ES_LDS["escm"]:
            for mode in R.ES_MODES:
                has_y, has_dout, _, _ = R.es_mode_args(mode)
                ref = R.ref64_escm(inp["praw"], inp["y"] if has_y else None, inp["dout3"] if has_dout else None, *w)
                got = _combine(lib, "escm", inp, mode, ld, w)
                _es_check(got, ref, "mml_escm_combine")
                if mode == "fused":
                    assert _es_same_bits(got, _combine(lib, "escm", inp, mode, ld, w))


@pytest.mark.parametrize("model", ["esmm", "escm"])
def test_combine_loss_propagates_nan(lib, model):
    """One NaN probability gives a NaN loss (torch.clamp keeps a NaN; as test_head_bce_loss_propagates_nan)."""
    inp, _ = R.build_escm(1025, 40)
    inp["praw"][1024, 0] = np.nan
    got = _combine(lib, model, inp, "fused", ES_LDS[model][0], () if model == "esmm" else (0.1, 1.0))
    assert np.isnan(got["loss"])
    assert np.isnan(got["pout"][1024, 0]) and np.isfinite(got["pout"][:1024]).all()


# ---------------------------------------------------------------------------------------------------------------
# DomainBN
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", R.DBN_DECAYS)
@pytest.mark.parametrize("B,n,D,degenerate", R.DBN_UPDATE_CASES)
def test_domain_bn_update(lib, B, n, D, degenerate, decay):
    """Population statistics over non-trivial priors within 1e-6 sum|terms| (Welford in double, one cast, three float32
    roundings: 4 x 2^-24); NaN exactly where the reference has it: the empty domain's mean and variance, the one-sample
    domain's variance ((7, 5, 4)).  (515, 300, 3): the second column block."""
    inp, census = R.build_domain_bn(B, n, D, seed=B + n, degenerate=degenerate)
    x, mask = Buf(B, n, n + 3, inp["x"]), Buf(B, D, D + 2, inp["mask"])
    pm, pv = Buf(D, n, data=inp["pop_mean"]), Buf(D, n, data=inp["pop_var"])
    ok(lib, lib.mml_domain_bn_update(x.ptr, x.ld, mask.ptr, mask.ld, B, n, D, pm.ptr, pv.ptr, float(F32(decay)), stream()))
    m, m_sa, v, v_sa = R.ref64_domain_bn_update(inp["x"], inp["mask"], inp["pop_mean"], inp["pop_var"], decay)
    assert int(np.isnan(m).sum()) == census["empty"] * n
    assert int(np.isnan(v).sum()) == (census["empty"] + census["single"]) * n
    assert_close_terms(pm.get("pop_mean"), m, m_sa, R.TOL_DBN_UPDATE, "mml_domain_bn_update: pop_mean")
    assert_close_terms(pv.get("pop_var"), v, v_sa, R.TOL_DBN_UPDATE, "mml_domain_bn_update: pop_var")


@pytest.mark.parametrize("B,n,D", R.DBN_EVAL_CASES)
def test_domain_bn_eval(lib, B, n, D):
    """The mask-weighted sum over the domains (soft rows, the all-zero row) within 1e-5 sum_d |mask term|;
    (4099, 130, 3) is the first size above 2048 x 256 threads.  A NaN domain gives NaN in every row."""
    inp, census = R.build_domain_bn(B, n, D, seed=B + n, soft=True)
    assert (B * n > 2048 * 256) == (B == 4099)
    x, mask = Buf(B, n, n + 3, inp["x"]), Buf(B, D, D + 2, inp["mask"])
    for nan_domain in (False, True):
        pmean = inp["pop_mean"].copy()
        if nan_domain:
            pmean[D - 1] = np.nan
        pm, pv, y = Buf(D, n, data=pmean), Buf(D, n, data=inp["pop_var"]), Buf(B, n, n + 5)
        ok(lib, lib.mml_domain_bn_eval(x.ptr, x.ld, mask.ptr, mask.ld, pm.ptr, pv.ptr, y.ptr, y.ld, B, n, D,
                                       float(F32(R.DBN_EPS)), stream()))
        ref, sa = R.ref64_domain_bn_eval(inp["x"], inp["mask"], pmean, inp["pop_var"], R.DBN_EPS)
        assert np.isnan(ref).all() == nan_domain
        assert_close_terms(y.get("y"), ref, sa, R.TOL_DBN_EVAL, "mml_domain_bn_eval: y")


# ---------------------------------------------------------------------------------------------------------------
# argument checks, one test per entry point: every pointer is a live buffer (65 536 floats) far larger than any extent
# the call names, so a missing check shows as a wrong return code, never as an access outside an allocation; the one
# accepted call at the end of each test shows that the refusals are due to the argument named in the comment
# ---------------------------------------------------------------------------------------------------------------
class Pool:
    def __init__(self):
        self.keep = []

    def __call__(self):
        t = torch.full((1 << 16,), 0.5, device=dev())
        self.keep.append(t)
        return t.data_ptr()


def refused(lib, rc, name):
    torch.cuda.synchronize()
    assert rc != 0, name + ": accepted"
    assert name in lib.mml_last_error().decode(), lib.mml_last_error()


def test_argument_checks_apg_features_fwd(lib):
    p, st, fn, name = Pool(), stream(), lib.mml_apg_features_fwd, "mml_apg_features_fwd"
    B, k, E = 4, 3, 2  # kE + k + E = 11
    refused(lib, fn(p(), k, p(), E, p(), 16, B, k, E, 10, st), name)   # Kf < kE + k + E
    refused(lib, fn(p(), k, p(), E, p(), 11, B, k, E, 12, st), name)   # ldz < Kf
    refused(lib, fn(p(), k, p(), E, p(), 12, -1, k, E, 12, st), name)  # B < 0
    refused(lib, fn(p(), k, p(), E, p(), 12, B, 0, E, 12, st), name)   # k = 0
    refused(lib, fn(p(), k, p(), E, p(), 12, B, k, 0, 12, st), name)   # E = 0
    assert fn(p(), k, p(), E, p(), 12, B, k, E, 12, st) == 0
    torch.cuda.synchronize()


def test_argument_checks_apg_features_bwd(lib):
    p, st, fn, name = Pool(), stream(), lib.mml_apg_features_bwd, "mml_apg_features_bwd"
    B, k, E = 4, 3, 2
    refused(lib, fn(p(), 8, p(), E, p(), k, B, k, E, 0, st), name)     # lddz < kE + k = 9
    refused(lib, fn(p(), 9, p(), E, p(), k, -1, k, E, 0, st), name)    # B < 0
    refused(lib, fn(p(), 9, p(), E, p(), k, B, 0, E, 0, st), name)     # k = 0
    assert fn(p(), 9, p(), E, p(), k, B, k, E, 0, st) == 0
    torch.cuda.synchronize()


def test_argument_checks_apg_weights(lib):
    p, st, fn, name = Pool(), stream(), lib.mml_apg_weights, "mml_apg_weights"
    k, E = 3, 2
    refused(lib, fn(p(), p(), p(), p(), 2, k, E, 0, 0, 0, 0, st), name)  # ldw < k
    refused(lib, fn(p(), p(), p(), p(), k, k, E, 2, 0, 0, 0, st), name)  # dir = 2
    refused(lib, fn(p(), p(), p(), p(), k, k, 0, 0, 0, 0, 0, st), name)  # E = 0
    assert fn(p(), p(), p(), p(), k, k, E, 1, 0, 0, 0, st) == 0
    torch.cuda.synchronize()


def test_argument_checks_snr_gate_weights_fwd(lib):
    p, st, fn, name = Pool(), stream(), lib.mml_snr_gate_weights_fwd, "mml_snr_gate_weights_fwd"
    be, ga, ep = _snr_consts()
    refused(lib, fn(p(), p(), p(), p(), 4, 10, 3, be, ga, ep, st), name)    # block % zw != 0
    refused(lib, fn(p(), p(), p(), p(), 4, 10, 0, be, ga, ep, st), name)    # zw = 0
    refused(lib, fn(p(), p(), p(), p(), 4, 10, 1, 0.0, ga, ep, st), name)   # beta = 0
    refused(lib, fn(p(), p(), p(), p(), -1, 10, 1, be, ga, ep, st), name)   # n_blocks < 0
    assert fn(p(), p(), p(), p(), 4, 10, 5, be, ga, ep, st) == 0
    torch.cuda.synchronize()


def test_argument_checks_snr_gate_weights_bwd(lib):
    p, st, fn, name = Pool(), stream(), lib.mml_snr_gate_weights_bwd, "mml_snr_gate_weights_bwd"
    be, ga, ep = _snr_consts()
    refused(lib, fn(p(), p(), p(), p(), p(), p(), 0, 0, 4, 10, 3, be, ga, ep, p(), st), name)    # block % zw != 0
    refused(lib, fn(p(), p(), p(), p(), p(), p(), 0, 0, 4, 10, 1, 0.0, ga, ep, p(), st), name)   # beta = 0
    refused(lib, fn(p(), p(), p(), p(), p(), p(), 0, 0, -1, 10, 1, be, ga, ep, p(), st), name)   # n_blocks < 0
    refused(lib, fn(p(), p(), p(), p(), None, p(), 0, 0, 4, 10, 1, be, ga, ep, p(), st), name)   # du = NULL with zw = 1
    assert fn(p(), p(), p(), p(), None, p(), 0, 0, 4, 10, 5, be, ga, ep, p(), st) == 0           # (fine for zw > 1)
    torch.cuda.synchronize()


def _combine_argument_checks(lib, fn, name, nout, extra):
    p, st, B = Pool(), stream(), 8
    refused(lib, fn(p(), 2, None, 2, None, nout, p(), nout, None, 2, p(), B, *extra, st), name)        # loss without y
    refused(lib, fn(p(), 1, None, 2, None, nout, p(), nout, None, 2, None, B, *extra, st), name)       # ldr < 2
    refused(lib, fn(p(), 2, None, 2, None, nout, p(), nout - 1, None, 2, None, B, *extra, st), name)   # ldo < 2 resp. 3
    refused(lib, fn(p(), 2, p(), 1, None, nout, p(), nout, None, 2, None, B, *extra, st), name)        # ldy < 2
    refused(lib, fn(p(), 2, None, 2, p(), nout - 1, p(), nout, p(), 2, None, B, *extra, st), name)     # lddo too small
    refused(lib, fn(p(), 2, p(), 2, None, nout, p(), nout, p(), 1, None, B, *extra, st), name)         # lddr < 2
    refused(lib, fn(p(), 2, None, 2, None, nout, p(), nout, None, 2, None, -1, *extra, st), name)      # B < 0
    assert fn(p(), 2, None, 2, None, nout, p(), nout, None, 2, None, B, *extra, st) == 0
    torch.cuda.synchronize()


def test_argument_checks_esmm_combine(lib):
    _combine_argument_checks(lib, lib.mml_esmm_combine, "mml_esmm_combine", 2, ())


def test_argument_checks_escm_combine(lib):
    _combine_argument_checks(lib, lib.mml_escm_combine, "mml_escm_combine", 3, (0.1, 1.0))


def test_argument_checks_domain_bn_update(lib):
    p, st, fn, name = Pool(), stream(), lib.mml_domain_bn_update, "mml_domain_bn_update"
    B, n, D = 8, 5, 3
    refused(lib, fn(p(), n, p(), D, B, n, 0, p(), p(), 0.9, st), name)        # D = 0
    refused(lib, fn(p(), n - 1, p(), D, B, n, D, p(), p(), 0.9, st), name)    # ldx < n
    refused(lib, fn(p(), n, p(), D - 1, B, n, D, p(), p(), 0.9, st), name)    # ldm < D
    refused(lib, fn(p(), n, p(), D, -1, n, D, p(), p(), 0.9, st), name)       # B < 0
    assert fn(p(), n, p(), D, B, n, D, p(), p(), 0.9, st) == 0
    torch.cuda.synchronize()


def test_argument_checks_domain_bn_eval(lib):
    p, st, fn, name = Pool(), stream(), lib.mml_domain_bn_eval, "mml_domain_bn_eval"
    B, n, D = 8, 5, 3
    refused(lib, fn(p(), n, p(), D, p(), p(), p(), n, B, n, 0, 1e-5, st), name)      # D = 0
    refused(lib, fn(p(), n - 1, p(), D, p(), p(), p(), n, B, n, D, 1e-5, st), name)  # ldx < n
    refused(lib, fn(p(), n, p(), D - 1, p(), p(), p(), n, B, n, D, 1e-5, st), name)  # ldm < D
    refused(lib, fn(p(), n, p(), D, p(), p(), p(), n - 1, B, n, D, 1e-5, st), name)  # ldy < n
    assert fn(p(), n, p(), D, p(), p(), p(), n, B, n, D, 1e-5, st) == 0
    torch.cuda.synchronize()
