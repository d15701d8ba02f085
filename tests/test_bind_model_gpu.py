"""The model-layer builders of mmlrec_amd/bind.py on the device: for every one of them, ONE call through
ops._issue(bind.X(...)) against the call spelled by hand as the kernel tests spell it (tests/test_model_kernels_gpu.py,
tests/test_kernels_gpu.py, tests/test_row_kernels_gpu.py, tests/test_pcgrad_gpu.py -- the independent statement of the
header's order), each on a fresh copy of the same inputs.  None of these kernels uses float atomics, their sums run in a
fixed order, so every buffer must come out bit-equal -- inputs included.  The cases are the smallest of the existing case
lists that have padded pitches (APG at B = 257, SNR (4, 3, 5, 1) and (6, 16, 16, 16), ESMM / ESCM at B = 65 with the second
pitch set, DomainBN (64, 16, 2) / (300, 16, 2), BatchNorm (300, 7, relu)); every matrix lives in the sentinel `Buf` of
tests/test_model_kernels_gpu.py with a pitch of its own, so a swapped pitch or pointer shows as a written padding column
or a changed input.  Dropout is also held to the oracle's mask."""
import numpy as np
import pytest
import torch

import model_kernel_refs as R
import row_kernel_refs as RR
import test_model_kernels_gpu as K
from model_kernel_refs import F32, bits_equal

pytestmark = pytest.mark.gpu
Buf, vec = K.Buf, K.vec


@pytest.fixture(scope="module")
def env():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, bind, ops
    return L.load(), ops, bind


def V(b):
    """The [rows, cols] view of a Buf (None stays None)."""
    return None if b is None else b.t[:b.rows, :b.cols]


def F(b):
    """The flat view of a one-row Buf."""
    return None if b is None else b.t[0, :b.cols]


def dev_t(a, dtype):
    return torch.tensor(a, dtype=dtype, device="cuda")


def both(env, make, built, hand, outs):
    """`built` (a list of Bounds, issued in order) and `hand` (the same launches spelled out: a list of return codes) on a
    fresh make() each; every buffer of the two sets must hold the same bits, and the outputs must have been written."""
    lib, ops, bind = env
    a, b = make(), make()
    for bound in built(bind, a):
        ops._issue(bound)
    for rc in hand(lib, b, K.stream()):
        K.ok(lib, rc)
    torch.cuda.synchronize()
    for k in a:
        if a[k] is None or k.startswith("_"):  # (_names: descriptor arrays that ride along)
            continue
        if isinstance(a[k], Buf):
            ga, gb = a[k].get("built " + k), b[k].get("hand " + k)
            assert bits_equal(ga, gb), k
            assert k not in outs or (ga.view(np.uint32) != K.SENT_BITS).any(), k + ": not written"
        else:
            assert torch.equal(a[k], b[k]), k
    return a


# ---- APG -------------------------------------------------------------------------------------------------------------
def test_apg_features(env):
    B, k, E, Kf = R.APG_FWD_CASES[1]
    assert (B, k, E) == R.APG_BWD_CASES[1] == (257, 5, 7)
    inp, _ = R.build_apg(B, k, E, seed=B + k)
    both(env, lambda: dict(o1=Buf(B, k, k + 3, inp["o1"]), s=Buf(B, E, E + 2, inp["s"]), z=Buf(B, Kf, Kf + 4)),
         lambda bind, d: [bind.apg_features_fwd(V(d["o1"]), V(d["s"]), V(d["z"]), k, E)],
         lambda lib, d, st: [lib.mml_apg_features_fwd(d["o1"].ptr, d["o1"].ld, d["s"].ptr, d["s"].ld, d["z"].ptr, d["z"].ld,
                                                      B, k, E, Kf, st)], outs=("z",))
    both(env, lambda: dict(dz=Buf(B, k * E + k, k * E + k + 1, inp["dz"]), s=Buf(B, E, E + 2, inp["s"]),
                           do1=Buf(B, k, k + 3, inp["prior"])),
         lambda bind, d: [bind.apg_features_bwd(V(d["dz"]), V(d["s"]), V(d["do1"]), k, E, True)],
         lambda lib, d, st: [lib.mml_apg_features_bwd(d["dz"].ptr, d["dz"].ld, d["s"].ptr, d["s"].ld, d["do1"].ptr,
                                                      d["do1"].ld, B, k, E, 1, st)], outs=("do1",))


def test_apg_weights(env):
    k, E = R.APG_W_CASES[1]
    w, c = R.build_apg_weights(k, E, seed=k + E)
    rows = c["rows"]
    both(env, lambda: dict(Wkk=Buf(k * k, E, data=w["Wkk"]), bkk=vec(w["bkk"]), Wb=Buf(k, E, data=w["Wb"]), Wcat=Buf(rows, k)),
         lambda bind, d: [bind.apg_weights(V(d["Wkk"]), F(d["bkk"]), V(d["Wb"]), V(d["Wcat"]), k, E, 0)],
         lambda lib, d, st: [lib.mml_apg_weights(d["Wkk"].ptr, d["bkk"].ptr, d["Wb"].ptr, d["Wcat"].ptr, k, k, E, 0, 0, 0, 0,
                                                 st)], outs=("Wcat",))
    flags = (1, 0, 0)  # (distinguishable: one target accumulates)
    assert flags in R.APG_W_FLAGS
    both(env, lambda: dict(dWkk=Buf(k * k, E, data=w["pWkk"]), dbkk=vec(w["pbkk"]), dWb=Buf(k, E, data=w["pWb"]),
                           dWcat=Buf(rows, k, data=w["dWcat"])),
         lambda bind, d: [bind.apg_weights(V(d["dWkk"]), F(d["dbkk"]), V(d["dWb"]), V(d["dWcat"]), k, E, 1, flags)],
         lambda lib, d, st: [lib.mml_apg_weights(d["dWkk"].ptr, d["dbkk"].ptr, d["dWb"].ptr, d["dWcat"].ptr, k, k, E, 1,
                                                 *flags, st)], outs=("dWkk", "dbkk", "dWb"))


# ---- SNR -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,rows,cols,zw", [R.SNR_CASES[3], R.SNR_CASES[4]])
def test_snr_gate_weights(env, nb, rows, cols, zw):
    inp, _ = R.build_snr(nb, rows, cols, zw, R.SNR_ALPHAS[1], seed=nb * 1000 + cols)
    block, consts = rows * cols, K._snr_consts()
    want_du = zw == 1  # (the frozen per-column u of MSSM takes no gradient: du = NULL)
    both(env, lambda: dict(u=vec(inp["u"]), al=vec(inp["alpha"]), M=vec(inp["M"]), W=Buf(1, nb * block, nb * block + 7)),
         lambda bind, d: [bind.snr_gate_weights_fwd(F(d["u"]), F(d["al"]), F(d["M"]), F(d["W"]), nb, block, zw, *consts)],
         lambda lib, d, st: [lib.mml_snr_gate_weights_fwd(d["u"].ptr, d["al"].ptr, d["M"].ptr, d["W"].ptr, nb, block, zw,
                                                          *consts, st)], outs=("W",))
    both(env, lambda: dict(dW=vec(inp["dW"]), M=vec(inp["M"]), u=vec(inp["u"]), al=vec(inp["alpha"]),
                           du=vec(inp["prior_du"]) if want_du else None, da=vec(inp["prior_dalpha"]), ws=Buf(1, nb, nb + 5)),
         lambda bind, d: [bind.snr_gate_weights_bwd(F(d["dW"]), F(d["M"]), F(d["u"]), F(d["al"]), F(d["du"]), F(d["da"]), 0,
                                                    1, nb, block, zw, *consts, F(d["ws"]))],
         lambda lib, d, st: [lib.mml_snr_gate_weights_bwd(d["dW"].ptr, d["M"].ptr, d["u"].ptr, d["al"].ptr, K.ptr(d["du"]),
                                                          d["da"].ptr, 0, 1, nb, block, zw, *consts, d["ws"].ptr, st)],
         outs=("da",) + (("du",) if want_du else ()))


# ---- ESMM / ESCM -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fused", "autograd"])
@pytest.mark.parametrize("model", ["esmm", "escm"])
def test_combine(env, model, mode):
    B = R.ES_B[3]
    ld = K.ES_LDS[model][1]
    has_y, has_dout, has_draw, has_loss = R.es_mode_args(mode)
    inp, _ = R.build_escm(B, R.esmm_npos(B))
    nout = 2 if model == "esmm" else 3
    wts = () if model == "esmm" else tuple(float(F32(x)) for x in R.ESCM_WEIGHTS[1])

    def make():
        return dict(praw=Buf(B, 2, ld["ldr"], inp["praw"]), y=Buf(B, 2, ld["ldy"], inp["y"]) if has_y else None,
                    dout=Buf(B, nout, ld["lddo"], inp["dout2" if model == "esmm" else "dout3"]) if has_dout else None,
                    pout=Buf(B, nout, ld["ldo"]), draw=Buf(B, 2, ld["lddr"]) if has_draw else None,
                    loss=Buf(1, 1, 4) if has_loss else None)

    def built(bind, d):
        fn = bind.esmm_combine if model == "esmm" else bind.escm_combine
        return [fn(V(d["praw"]), V(d["y"]), V(d["dout"]), V(d["pout"]), V(d["draw"]), F(d["loss"]), B, *wts)]

    def hand(lib, d, st):
        fn = lib.mml_esmm_combine if model == "esmm" else lib.mml_escm_combine
        return [fn(d["praw"].ptr, ld["ldr"], K.ptr(d["y"]), ld["ldy"], K.ptr(d["dout"]), ld["lddo"], d["pout"].ptr, ld["ldo"],
                   K.ptr(d["draw"]), ld["lddr"], K.ptr(d["loss"]), B, *wts, st)]

    both(env, make, built, hand, outs=("pout", "draw") + (("loss",) if has_loss else ()))


# ---- BatchNorm / DomainBN ---------------------------------------------------------------------------------------------
def test_domain_bn(env):
    B, n, D, _ = R.DBN_UPDATE_CASES[0]
    inp, _ = R.build_domain_bn(B, n, D, seed=B + n)
    decay = float(F32(R.DBN_DECAYS[0]))
    both(env, lambda: dict(x=Buf(B, n, n + 3, inp["x"]), mask=Buf(B, D, D + 2, inp["mask"]),
                           pm=Buf(D, n, data=inp["pop_mean"]), pv=Buf(D, n, data=inp["pop_var"])),
         lambda bind, d: [bind.domain_bn_update(V(d["x"]), V(d["mask"]), V(d["pm"]), V(d["pv"]), decay)],
         lambda lib, d, st: [lib.mml_domain_bn_update(d["x"].ptr, d["x"].ld, d["mask"].ptr, d["mask"].ld, B, n, D, d["pm"].ptr,
                                                      d["pv"].ptr, decay, st)], outs=("pm", "pv"))
    B, n, D = R.DBN_EVAL_CASES[0]
    inp, _ = R.build_domain_bn(B, n, D, seed=B + n, soft=True)
    eps = float(F32(R.DBN_EPS))
    both(env, lambda: dict(x=Buf(B, n, n + 3, inp["x"]), mask=Buf(B, D, D + 2, inp["mask"]),
                           pm=Buf(D, n, data=inp["pop_mean"]), pv=Buf(D, n, data=inp["pop_var"]), y=Buf(B, n, n + 5)),
         lambda bind, d: [bind.domain_bn_eval(V(d["x"]), V(d["mask"]), V(d["pm"]), V(d["pv"]), V(d["y"]), eps)],
         lambda lib, d, st: [lib.mml_domain_bn_eval(d["x"].ptr, d["x"].ld, d["mask"].ptr, d["mask"].ld, d["pm"].ptr,
                                                    d["pv"].ptr, d["y"].ptr, d["y"].ld, B, n, D, eps, st)], outs=("y",))


def test_batchnorm(env):
    """Forward in training mode (running statistics and the batch counter move), then the backward over what it left."""
    lib = env[0]
    B, n = 300, 7  # (the smallest case of tests/test_kernels_gpu.py::test_batchnorm_fwd_bwd)
    rng = np.random.default_rng(B + n)
    z = (rng.standard_normal((B, n)) * 2 + 0.5).astype(F32)
    gamma, beta = (1 + 0.2 * rng.standard_normal(n)).astype(F32), (0.1 * rng.standard_normal(n)).astype(F32)
    rm0, rv0 = rng.standard_normal(n).astype(F32), (1 + rng.random(n)).astype(F32)
    dy = rng.standard_normal((B, n)).astype(F32)
    nbytes = int(lib.mml_bn_workspace_bytes(B, n))
    act = 1  # relu

    def make():
        return dict(z=Buf(B, n, n + 5, z), g=vec(gamma), b=vec(beta), rm=vec(rm0), rv=vec(rv0), mean=vec(np.zeros(n)),
                    rstd=vec(np.zeros(n)), y=Buf(B, n, n + 2), dy=Buf(B, n, n + 3, dy), dz=Buf(B, n, n + 1),
                    dg=vec(np.ones(n)), db=vec(np.ones(n)), nbt=dev_t([3], torch.int64),
                    ws=torch.zeros(max(nbytes, 4), dtype=torch.uint8, device="cuda"))

    def built(bind, d):
        return [bind.bn_fwd(V(d["z"]), F(d["g"]), F(d["b"]), F(d["rm"]), F(d["rv"]), d["nbt"], F(d["mean"]), F(d["rstd"]),
                            V(d["y"]), act, True, 1e-5, 0.1, d["ws"]),
                bind.bn_bwd(V(d["dy"]), V(d["z"]), F(d["g"]), F(d["mean"]), F(d["rstd"]), V(d["dz"]), F(d["dg"]), F(d["db"]),
                            True, d["ws"])]

    def hand(lib, d, st):
        return [lib.mml_bn_fwd(d["z"].ptr, d["z"].ld, d["g"].ptr, d["b"].ptr, d["rm"].ptr, d["rv"].ptr, d["nbt"].data_ptr(),
                               d["mean"].ptr, d["rstd"].ptr, d["y"].ptr, d["y"].ld, B, n, act, 1, 1e-5, 0.1,
                               d["ws"].data_ptr(), d["ws"].numel(), st),
                lib.mml_bn_bwd(d["dy"].ptr, d["dy"].ld, d["z"].ptr, d["z"].ld, d["g"].ptr, d["mean"].ptr, d["rstd"].ptr,
                               d["dz"].ptr, d["dz"].ld, d["dg"].ptr, d["db"].ptr, 1, B, n, d["ws"].data_ptr(),
                               d["ws"].numel(), st)]

    got = both(env, make, built, hand, outs=("y", "mean", "rstd", "dz", "dg", "db", "rm", "rv"))
    assert int(got["nbt"].item()) == 4
    assert not bits_equal(got["rm"].get("rm")[0], rm0) and not bits_equal(got["dg"].get("dg")[0], np.ones(n, F32))


# ---- dropout ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [0, 1])
def test_dropout(env, accumulate):
    from oracle import mmlrec_oracle as orc
    rows, cols, p, step, row0 = 257, 37, 0.3, 5, 11
    seed, site = 0xfeedfacecafebeef, 0x9e3779b9
    rng = np.random.default_rng(rows + cols)
    x, prior = rng.standard_normal((rows, cols)).astype(F32), rng.standard_normal((rows, cols)).astype(F32)
    got = both(env, lambda: dict(x=Buf(rows, cols, cols + 3, x), out=Buf(rows, cols, cols + 1, prior),
                                 sd=dev_t([step], torch.int32)),
               lambda bind, d: [bind.dropout(V(d["x"]), V(d["out"]), p, seed, site, d["sd"], 99, accumulate, row0)],
               lambda lib, d, st: [lib.mml_dropout(d["x"].ptr, d["x"].ld, d["out"].ptr, d["out"].ld, rows, cols, row0, p, seed,
                                                   site, d["sd"].data_ptr(), 99, accumulate, st)], outs=("out",))
    want = x * orc.dropout_scale(rows, cols, p, seed, step, site, row0=row0)
    if accumulate:
        want = (want + prior).astype(F32)
    assert bits_equal(got["out"].get("out"), want)


# ---- element-wise, copies ---------------------------------------------------------------------------------------------
def test_elementwise(env):
    n = RR.EW_LENGTHS[2]
    assert n == 257
    w = RR.build_ew(n, n)
    rng = np.random.default_rng(n)
    bh = RR.act_outputs(RR.ACT_SIGMOID2, n, rng)
    ah = RR.act_outputs(RR.ACT_RELU, n, rng)
    zeros = np.zeros(n, F32)
    both(env, lambda: dict(a=vec(w["a"]), b=vec(w["b"]), out=vec(zeros)),
         lambda bind, d: [bind.ew_mul(F(d["a"]), F(d["b"]), F(d["out"]))],
         lambda lib, d, st: [lib.mml_ew_mul(d["a"].ptr, d["b"].ptr, d["out"].ptr, n, st)], outs=("out",))
    both(env, lambda: dict(d=vec(w["d"]), a=vec(w["a"]), b=vec(w["b"]), da=vec(w["pa"]), db=vec(w["pb"])),
         lambda bind, d: [bind.ew_mul_bwd(F(d["d"]), F(d["a"]), F(d["b"]), F(d["da"]), F(d["db"]), True, False)],
         lambda lib, d, st: [lib.mml_ew_mul_bwd(d["d"].ptr, d["a"].ptr, d["b"].ptr, d["da"].ptr, d["db"].ptr, 1, 0, n, st)],
         outs=("da", "db"))
    both(env, lambda: dict(d=vec(w["d"]), a=vec(ah), b=vec(bh), da=vec(zeros), db=vec(zeros)),
         lambda bind, d: [bind.ew_mul_bwd_act(F(d["d"]), F(d["a"]), F(d["b"]), F(d["da"]), F(d["db"]), 0, 0, RR.ACT_RELU,
                                              RR.ACT_SIGMOID2)],
         lambda lib, d, st: [lib.mml_ew_mul_bwd_act(d["d"].ptr, d["a"].ptr, d["b"].ptr, d["da"].ptr, d["db"].ptr, 0, 0, n,
                                                    RR.ACT_RELU, RR.ACT_SIGMOID2, st)], outs=("da", "db"))
    both(env, lambda: dict(a=vec(w["a"]), b=vec(w["b"]), c=vec(w["d"]), out=vec(w["pa"], pad=5)),
         lambda bind, d: [bind.ew_add_n([F(d["a"]), F(d["b"]), F(d["c"])], F(d["out"]))],
         lambda lib, d, st: [lib.mml_ew_add_n(env[1]._ptr_array([F(d[k]) for k in "abc"]), 3, d["out"].ptr, n, st)],
         outs=("out",))
    both(env, lambda: dict(y=vec(bh), dy=vec(w["d"]), dst=vec(zeros, pad=4)),
         lambda bind, d: [bind.act_bwd(F(d["y"]), F(d["dy"]), F(d["dst"]), RR.ACT_SIGMOID2)],
         lambda lib, d, st: [lib.mml_act_bwd(d["y"].ptr, d["dy"].ptr, d["dst"].ptr, n, RR.ACT_SIGMOID2, st)], outs=("dst",))


def test_copies(env):
    rows, cols, n = 37, 5, 257
    rng = np.random.default_rng(cols)
    s2, d2 = rng.standard_normal((rows, cols)).astype(F32), rng.standard_normal((rows, cols)).astype(F32)
    both(env, lambda: dict(src=Buf(rows, cols, cols + 3, s2), dst=Buf(rows, cols, cols + 2, d2)),
         lambda bind, d: [bind.copy2d(V(d["src"]), V(d["dst"]), True)],
         lambda lib, d, st: [lib.mml_copy2d(d["src"].ptr, d["src"].ld, d["dst"].ptr, d["dst"].ld, rows, cols, 1, st)],
         outs=("dst",))
    s1, d1 = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    for acc in (0, 1):
        both(env, lambda: dict(src=vec(s1), dst=vec(d1, pad=5)),
             lambda bind, d: [bind.copy_flat(F(d["src"]), F(d["dst"]), acc)],
             lambda lib, d, st: [lib.mml_copy2d(d["src"].ptr, n, d["dst"].ptr, n, 1, n, acc, st)], outs=("dst",))


# ---- PCGrad, counters -------------------------------------------------------------------------------------------------
def test_pcgrad(env):
    lib, ops, bind = env
    T = 3
    rng = np.random.default_rng(7)
    host = dict(flat=rng.standard_normal((T, 257)).astype(F32), tab=rng.standard_normal((T, 100, 8)).astype(F32),
                odd=rng.standard_normal((T, 77, 5)).astype(F32))
    order = [[0, 1, 2], [2, 1, 0], [1, 0, 2]]

    def make():
        t = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        marks = torch.zeros(100, dtype=torch.uint8, device="cuda")
        marks[::7] = 1
        out = {k: torch.full(tuple(v.shape[1:]), 7.0, device="cuda") for k, v in host.items()}
        segs = [dict(banks=list(t["flat"]), out=out["flat"]), dict(banks=list(t["tab"]), out=out["tab"], marks=marks),
                dict(banks=[t["odd"][0], None, t["odd"][2]], out=out["odd"])]
        arr = ops.make_pcgrad_segs(segs, T, need_out=True)
        stash = ops.make_pcgrad_segs([dict(banks=[t["tab"][1]], out=t["tab"][2], marks=marks)], 1, need_out=True)
        nws = int(lib.mml_pcgrad_workspace_bytes(arr, len(segs), T))
        return dict(t_flat=t["flat"], t_tab=t["tab"], t_odd=t["odd"], o_flat=out["flat"], o_tab=out["tab"], o_odd=out["odd"],
                    marks=marks, gram=torch.zeros(T, T, dtype=torch.float64, device="cuda"),
                    order=dev_t(order, torch.int32), w=torch.zeros(2 * T, device="cuda"),
                    fired=torch.full((T, T), -1, dtype=torch.int32, device="cuda"),
                    ws=torch.zeros(max(nws, 256), dtype=torch.uint8, device="cuda"), _arr=(arr, stash, len(segs)))

    def built(bind, d):
        arr, stash, n = d["_arr"]
        return [bind.pcgrad_gram(arr, n, T, d["gram"], d["ws"]), bind.pcgrad_weights(d["gram"], d["order"], T, d["w"], d["fired"]),
                bind.pcgrad_combine(arr, n, T, d["w"]), bind.pcgrad_stash(stash, 1, True)]

    def hand(lib, d, st):
        arr, stash, n = d["_arr"]
        return [lib.mml_pcgrad_gram(arr, n, T, d["gram"].data_ptr(), d["ws"].data_ptr(), d["ws"].numel(), st),
                lib.mml_pcgrad_weights(d["gram"].data_ptr(), d["order"].data_ptr(), T, d["w"].data_ptr(),
                                       d["fired"].data_ptr(), st),
                lib.mml_pcgrad_combine(arr, n, T, d["w"].data_ptr(), st), lib.mml_pcgrad_stash(stash, 1, 1, st)]

    got = both(env, make, built, hand, outs=())
    assert bool((got["gram"].diagonal() > 0).all()) and bool((got["fired"] >= 0).all()) and bool((got["w"] != 0).all())
    assert bool((got["o_flat"] != 7.0).all()) and bool((got["o_tab"][::7] != 7.0).all()) and bool((got["o_tab"][1] == 7.0).all())
    assert not bool(got["t_tab"][1][::7].any()) and bool(got["t_tab"][1][1].any())  # stashed rows: moved and cleared


def test_counters(env):
    def make():
        return dict(c=dev_t([5], torch.int32), r=dev_t([9], torch.int32),
                    pool=torch.full((4, 8), 7, dtype=torch.int32, device="cuda"))

    d = both(env, make,
             lambda bind, d: [bind.counter_update(d["c"], 3, False), bind.counter_update(d["r"], 0, True),
                              bind.amax_reset(d["pool"], 3)],
             lambda lib, d, st: [lib.mml_counter_update(d["c"].data_ptr(), 3, 0, st),
                                 lib.mml_counter_update(d["r"].data_ptr(), 0, 1, st),
                                 lib.mml_amax_reset(d["pool"].data_ptr(), 3, st)], outs=())
    assert int(d["c"].item()) == 8 and int(d["r"].item()) == 0
    assert not bool(d["pool"][:3].any()) and bool((d["pool"][3] == 7).all())
