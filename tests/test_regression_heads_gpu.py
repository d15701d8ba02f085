"""Head kinds (include/mmlrec.h K5: MML_HEAD_KIND -- identity output, squared / absolute error) in the three head kernels:
the fast row kernel (csrc/rows_fast.hip, plain, gated and dh_bf16), the general row kernel (csrc/gate_head.hip) and the fused
tower + head kernel (csrc/tower_head.hip), each against a float64 restatement written here.

Expressions (logit z, mask value m, label y): p = sigmoid(z) or z; stored prediction pm = p m; dz = d(pm) m p (1 - p) or
d(pm) m; BCE as before, MSE (pm - y)^2 with d(pm) = 2 (pm - y), MAE |pm - y| with d(pm) = sign(pm - y), sign(0) = 0.

Criteria: those of tests/test_tower_head_gpu.py, which already applies them to the same arithmetic (max-norm relative
1e-5; 2e-5 for dw and dbias; 1e-4 for the summed loss).  Nothing here was widened for identity outputs.  dh_bf16: the
stored dH is a bf16 rounding (8 significant bits, round to nearest: half an ulp = 2^-8 relative) of the same fp32 value,
so 2^-8 + 1e-5.

Labels of MAE heads are the float64 prediction +- (0.05 + u), u uniform in [0, 1): the sign of pm - y is never in doubt and
no sample is excluded.  Separately a handful of samples get y set to the bits of the prediction an earlier call returned
(mml_head_fwd for the row kernels; a first launch for the fused kernel, which has no forward-only entry): their error is
exactly zero, and their dH rows must be exactly zero under MSE and MAE alike.  The float64 restatement takes the label as
the prediction on those rows (zero error by construction): its own prediction differs from the kernel's in the last bits,
and the sign of that difference is not a gradient.
"""
import pytest

pytestmark = pytest.mark.gpu

SIG, IDN = 0, 1
BCE, MSE, MAE = 0, 1, 2
# kinds a group cycles through (output form, loss): every allowed pair
KINDS = [(IDN, MSE), (SIG, BCE), (IDN, MAE), (SIG, MSE), (SIG, MAE)]
ZERO_ROWS = [0, 3, 17, 30, 31]   # samples whose label is set to the prediction's own bits (all < 32 <= every B here)


@pytest.fixture()
def env():
    import torch
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, ops
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    lib = L.load()
    mode0 = lib.mml_gemm_get_mode()
    lib.mml_gemm_set_mode(4)
    yield torch, L, ops, lib
    lib.mml_gemm_set_mode(mode0)


def rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))


def kinds_for(T, first):
    return [KINDS[(first + t) % len(KINDS)] for t in range(T)]


# ------------------------------------------------------------------------------------------------ float64 restatement
def chain64(torch, z64, m, kind, y=None, dprob=None, zero_rows=None):
    """(pm, loss terms or None, dz) in float64 from the logit, the way the kernels round: the logit and the stored
    prediction are fp32 values."""
    out, lk = kind
    z = z64.float().double()
    p = z if out == IDN else 1.0 / (1.0 + torch.exp(-z))
    pm = (p * m).float().double()
    err = None
    if y is not None:
        err = pm - y
        if zero_rows is not None and lk != BCE:  # the label is the stored prediction itself: no error
            err[zero_rows] = 0.0
    if y is None:
        dpm, terms = dprob.double(), None
    elif lk == MSE:
        terms, dpm = err ** 2, 2.0 * err
    elif lk == MAE:
        terms, dpm = err.abs(), torch.sign(err)
    else:
        lp = torch.clamp(torch.log(pm.float()), min=-100).double()
        l1p = torch.clamp(torch.log1p(-pm.float()), min=-100).double()
        terms = -(y * lp + (1 - y) * l1p)
        dpm = (pm - y) / torch.clamp(pm * (1 - pm), min=1e-12)
    dz = dpm * m if out == IDN else dpm * m * p * (1 - p)
    return pm, terms, dz


def gate_deriv(L, g, act):
    if act == L.ACT_SIGMOID:
        return g * (1 - g)
    if act == L.ACT_SIGMOID2:
        return g * (1 - 0.5 * g)
    return g * 0 + 1


def head_logit64(q):
    x = q["Hin"].double()
    if q.get("gate") is not None:
        x = x * q["gate"].double()
    w = q["w"].double()
    return x, x @ w + q["bias"].double() + (q["bias2"].double().sum() if q.get("bias2") is not None else 0.0)


def head_reference(torch, L, q, m, kind, y=None, dprob=None):
    x, z = head_logit64(q)
    pm, terms, dz = chain64(torch, z, m, kind, y, dprob, zero_rows=ZERO_ROWS)
    w = q["w"].double()
    dH = dz[:, None] * w[None, :]
    dG = None
    if q.get("gate") is not None:
        g = q["gate"].double()
        dG = dH * q["Hin"].double() * gate_deriv(L, g, q["gate_act"])
        dH = dH * g
    if q["h_relu"]:
        dH = dH * (q["Hin"].double() > 0)
    return pm, terms, dH, dG, dz @ x, float(dz.sum())


# ------------------------------------------------------------------------------------------------ row kernels
def build_heads(torch, L, B, H, T, masked, gated, h_relu, kinds, seed):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(seed)
    mask = (torch.rand(B, 2, generator=g) < 0.6).float().to(dev) if masked else None
    acts = [L.ACT_SIGMOID2, L.ACT_NONE, L.ACT_SIGMOID]
    heads = []
    for t in range(T):
        Hin = torch.randn(B, H, generator=g).to(dev)
        q = dict(Hin=Hin, w=(torch.randn(H, generator=g) / H ** 0.5).to(dev), bias=torch.randn(1, generator=g).to(dev),
                 bias2=(torch.randn(2, generator=g) * 0.1).to(dev) if t % 2 else None, h_relu=h_relu,
                 mask_col=(t % 2 if masked else -1), kind=L.head_kind(*kinds[t]))
        if gated and t != 1:  # (head 1 of a gated group stays plain: the flag is per head)
            act = acts[t % 3]
            raw = torch.randn(B, H, generator=g)
            gate = raw if act == L.ACT_NONE else (torch.sigmoid(raw) * (2.0 if act == L.ACT_SIGMOID2 else 1.0))
            q.update(gate=gate.to(dev), gate_act=act)
        heads.append(q)
    return mask, heads, g


def mask_of(torch, mask, q, B):
    return mask[:, q["mask_col"]].double() if q["mask_col"] >= 0 else torch.ones(B, dtype=torch.float64, device="cuda:0")


def fresh_outputs(torch, heads, B, bf16=False):
    dev = torch.device("cuda:0")
    nan = float("nan")
    for q in heads:
        H = q["Hin"].shape[1]
        q["dH"] = torch.full((B, H), nan, device=dev, dtype=torch.bfloat16 if bf16 else torch.float32)
        q["dw"], q["dbias"] = torch.full((H,), nan, device=dev), torch.full((1,), nan, device=dev)
        if q.get("gate") is not None:
            q["dgate"] = torch.full((B, H), nan, device=dev)


def make_labels(torch, L, heads, mask, kinds, B, gen, prob_fwd):
    """Binary labels for BCE heads, continuous ones for MSE heads, prediction +- (0.05 + u) for MAE heads; the rows of
    ZERO_ROWS of every non-BCE head: the bits of the forward-only prediction."""
    dev = torch.device("cuda:0")
    y = torch.empty(B, len(heads), device=dev)
    for t, q in enumerate(heads):
        out, lk = kinds[t]
        if lk == BCE:
            y[:, t] = (torch.rand(B, generator=gen) < 0.4).float().to(dev)
            continue
        if lk == MSE:
            y[:, t] = (torch.randn(B, generator=gen) * 1.5 + 0.3).to(dev)
        else:
            _, z = head_logit64(q)
            pm, _, _ = chain64(torch, z, mask_of(torch, mask, q, B), (out, lk), dprob=z * 0)
            s = (torch.rand(B, generator=gen) < 0.5).double().to(dev) * 2 - 1
            y[:, t] = (pm + s * (0.05 + torch.rand(B, generator=gen).double().to(dev))).float()
        y[ZERO_ROWS, t] = prob_fwd[ZERO_ROWS, t]
    return y


def check_heads(torch, L, heads, mask, kinds, B, prob, loss, y=None, dprob=None, dh_tol=1e-5):
    total = 0.0
    for t, q in enumerate(heads):
        m = mask_of(torch, mask, q, B)
        pm, terms, dH, dG, dw, db = head_reference(torch, L, q, m, kinds[t], None if y is None else y[:, t].double(),
                                                   None if dprob is None else dprob[:, t])
        assert rel(prob[:, t], pm) < 1e-5, (t, kinds[t], rel(prob[:, t], pm))
        assert rel(q["dH"].float(), dH) < dh_tol, (t, kinds[t], rel(q["dH"].float(), dH))
        if dG is not None:
            assert rel(q["dgate"], dG) < 1e-5, (t, kinds[t], rel(q["dgate"], dG))
        assert rel(q["dw"], dw) < 2e-5, (t, kinds[t], rel(q["dw"], dw))
        assert abs(float(q["dbias"]) - db) < 2e-5 * max(abs(db), 1.0), (t, kinds[t])
        if terms is not None:
            total += float(terms.sum())
            if kinds[t][1] != BCE:  # label = the prediction's own bits: no error, no gradient, exactly
                assert float(q["dH"].float()[ZERO_ROWS].abs().max()) == 0.0, (t, kinds[t])
                if dG is not None:
                    assert float(q["dgate"][ZERO_ROWS].abs().max()) == 0.0, (t, kinds[t])
    if y is not None:
        assert abs(float(loss) - total) / total < 1e-4, (float(loss), total)


ROW_CASES = [
    # B, H, T, masked, gated, h_relu, first kind
    (32, 16, 1, False, False, 1, 0),
    (32, 16, 1, False, False, 0, 2),
    (333, 64, 2, True, False, 0, 0),
    (8192 + 77, 128, 3, False, True, 1, 1),
    (65536, 64, 2, True, False, 1, 4),
    (4099, 256, 8, True, False, 1, 0),
    (16384, 64, 4, True, True, 1, 2),
    (1000, 32, 5, False, True, 0, 3),
    (65536, 128, 4, False, False, 1, 0),
    # H = 50: not a multiple of 4 -> the general row kernel
    (333, 50, 3, True, False, 1, 0),
    (65536, 50, 2, False, False, 1, 2),
    (32, 50, 8, True, False, 0, 1),
]


@pytest.mark.parametrize("B,H,T,masked,gated,h_relu,first", ROW_CASES)
def test_row_kernels_match_float64(env, B, H, T, masked, gated, h_relu, first):
    torch, L, ops, lib = env
    dev = torch.device("cuda:0")
    kinds = kinds_for(T, first)
    mask, heads, gen = build_heads(torch, L, B, H, T, masked, gated, h_relu, kinds, seed=B + H + T + first)
    # forward only: the output form
    prob_fwd = torch.full((B, T), float("nan"), device=dev)
    ops.head_fwd(ops.make_head_group(heads, prob_fwd, mask=mask))
    for t, q in enumerate(heads):
        _, z = head_logit64(q)
        pm, _, _ = chain64(torch, z, mask_of(torch, mask, q, B), kinds[t], dprob=z * 0)
        assert rel(prob_fwd[:, t], pm) < 1e-5, (t, kinds[t])
    y = make_labels(torch, L, heads, mask, kinds, B, gen, prob_fwd)
    # labels: one call
    fresh_outputs(torch, heads, B)
    prob, loss = torch.full((B, T), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev)
    ops.head_bce_fwd_bwd(ops.make_head_group(heads, prob, y=y, mask=mask, loss=loss), dev)
    torch.cuda.synchronize()
    assert torch.equal(prob, prob_fwd)  # the forward-only entry and the training entry agree to the bit
    check_heads(torch, L, heads, mask, kinds, B, prob, loss, y=y)
    one_call = [(q["dH"].clone(), q["dw"].clone(), q["dbias"].clone()) for q in heads]
    # labels: phase 1, then the reduction through mml_rows_reduce_batch
    fresh_outputs(torch, heads, B)
    prob2, loss2 = torch.full((B, T), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev)
    ops.rows_phase1_then_batched_reduce([ops.make_head_group(heads, prob2, y=y, mask=mask, loss=loss2)], [], dev)
    torch.cuda.synchronize()
    check_heads(torch, L, heads, mask, kinds, B, prob2, loss2, y=y)
    for q, (dh, dw, db) in zip(heads, one_call):
        assert torch.equal(q["dH"], dh)
    # dprob instead of labels: only the output form matters
    dprob = torch.randn(B, T, generator=gen).to(dev)
    fresh_outputs(torch, heads, B)
    prob3 = torch.full((B, T), float("nan"), device=dev)
    ops.head_bce_fwd_bwd(ops.make_head_group(heads, prob3, mask=mask, dprob=dprob), dev)
    torch.cuda.synchronize()
    check_heads(torch, L, heads, mask, kinds, B, prob3, None, dprob=dprob)
    # bf16 dH (fast kernel, plain heads)
    if H % 8 == 0 and not gated:
        fresh_outputs(torch, heads, B, bf16=True)
        prob4, loss4 = torch.full((B, T), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev)
        ops.head_bce_fwd_bwd(ops.make_head_group(heads, prob4, y=y, mask=mask, loss=loss4), dev)
        torch.cuda.synchronize()
        check_heads(torch, L, heads, mask, kinds, B, prob4, loss4, y=y, dh_tol=2.0 ** -8 + 1e-5)


# ------------------------------------------------------------------------------------------------ fused tower + head
RELU_EDGE = 1e-5  # tests/test_tower_head_gpu.py holds the forward GEMM's arithmetic to 1e-5 of the largest value


def tower_reference(torch, y, mask, q, t, kind, zero_rows=None, got_dH=None):
    """relu'(h) of an element whose float64 pre-activation lies inside the forward GEMM's own error (RELU_EDGE times the
    largest pre-activation) is decided by neither side; one such element costs a whole |dlogit w| in the max-norm.  With
    got_dH the restatement takes the kernel's choice there (either is a correct derivative) and carries it through dA;
    the caller asserts how few such elements there are."""
    A, W = q["A"].double(), q["W"].double()
    pre = A @ W.t() + q["bias1"].double()
    h = torch.relu(pre)
    on = pre > 0
    edge = pre.abs() < RELU_EDGE * pre.abs().max()
    if got_dH is not None:
        on = torch.where(edge, got_dH != 0, on)
    z = h @ q["w"].double() + q["hbias"].double()
    m = mask[:, q["mask_col"]].double() if q["mask_col"] >= 0 else torch.ones_like(z)
    pm, terms, dz = chain64(torch, z, m, kind, y[:, t].double(), zero_rows=zero_rows)
    dH = dz[:, None] * q["w"].double()[None, :] * on
    tower_reference.edge_count = int(edge.sum())
    return pm, float(terms.sum()), dH, dH @ W, dz @ h, float(dz.sum())


def tower_labels(torch, y, mask, tasks, kinds, M, gen, prob_first):
    dev = torch.device("cuda:0")
    for t, q in enumerate(tasks):
        out, lk = kinds[t]
        if lk == BCE:
            continue
        if lk == MSE:
            y[:, t] = (torch.randn(M, generator=gen) * 1.5 + 0.3).to(dev)
        else:
            pm = tower_reference(torch, y * 0, mask, q, t, (out, MSE))[0]
            s = (torch.rand(M, generator=gen) < 0.5).double().to(dev) * 2 - 1
            y[:, t] = (pm + s * (0.05 + torch.rand(M, generator=gen).double().to(dev))).float()
        y[ZERO_ROWS, t] = prob_first[ZERO_ROWS, t]


@pytest.mark.parametrize("M,K,T,masked,scale,first", [(65536, 128, 2, True, 1.0, 1), (8192 + 77, 128, 2, False, 1e-3, 0),
                                                      (333, 128, 4, True, 1.0, 2), (16384, 64, 3, False, 30.0, 0),
                                                      (32, 128, 1, False, 1.0, 0), (32768, 128, 8, True, 1.0, 0)])
def test_tower_head_matches_float64(env, M, K, T, masked, scale, first):
    from test_tower_head_gpu import build
    torch, L, ops, lib = env
    dev = torch.device("cuda:0")
    N = 64
    kinds = kinds_for(T, first)
    y, mask, tasks = build(torch, L, ops, M, K, N, T, masked, seed=M + K + T + 1, scale=scale)
    for t, q in enumerate(tasks):
        q["kind"] = L.head_kind(*kinds[t])
    gen = torch.Generator(device="cpu").manual_seed(M + T)
    # a first launch (labels of non-BCE heads still binary: only its predictions are used)
    prob0 = torch.full((M, T), float("nan"), device=dev)
    grp0 = ops.make_tower_head_group(tasks, prob0, y, mask=mask, loss=torch.zeros(1, device=dev))
    assert lib.mml_tower_head_serves(grp0) == 1
    ops.tower_head_fwd_bwd(grp0, dev)
    torch.cuda.synchronize()
    tower_labels(torch, y, mask, tasks, kinds, M, gen, prob0)
    prob = torch.full((M, T), float("nan"), device=dev)
    loss = torch.full((1,), float("nan"), device=dev)
    for q in tasks:
        for k in ("dH", "dA", "dw", "dhbias"):
            q[k].fill_(float("nan"))
        q["amax_dH"].zero_()
        q["amax_dA"].zero_()
    grp = ops.make_tower_head_group(tasks, prob, y, mask=mask, loss=loss)
    ops.tower_head_fwd_bwd(grp, dev)
    torch.cuda.synchronize()
    assert torch.equal(prob, prob0)
    total = 0.0
    for t, q in enumerate(tasks):
        pm, ls, dH, dA, dw, db = tower_reference(torch, y, mask, q, t, kinds[t], zero_rows=ZERO_ROWS, got_dH=q["dH"])
        total += ls
        # (a standard-normal-like pre-activation lies inside the edge with probability ~ RELU_EDGE: a handful per tensor)
        assert tower_reference.edge_count <= 1 + 1e-4 * q["dH"].numel(), tower_reference.edge_count
        assert rel(prob[:, t], pm) < 1e-5, (t, kinds[t], rel(prob[:, t], pm))
        assert rel(q["dH"], dH) < 1e-5, (t, kinds[t], rel(q["dH"], dH))
        assert rel(q["dA"], dA) < 1e-5, (t, kinds[t], rel(q["dA"], dA))
        assert rel(q["dw"], dw) < 2e-5, (t, kinds[t], rel(q["dw"], dw))
        assert abs(float(q["dhbias"]) - db) < 2e-5 * max(abs(db), 1.0)
        if kinds[t][1] != BCE:
            assert float(q["dH"][ZERO_ROWS].abs().max()) == 0.0 and float(q["dA"][ZERO_ROWS].abs().max()) == 0.0
        for buf, slot in ((q["dH"], q["amax_dH"]), (q["dA"], q["amax_dA"])):
            am = float(torch.max(slot.view(torch.float32)))
            assert am >= float(buf.abs().max()) and am <= float(buf.abs().max()) * (1 + 1e-6)
    assert abs(float(loss) - total) / total < 1e-4
    # the two-launch form: the same bits
    keep = [(q["dw"].clone(), q["dhbias"].clone(), q["dH"].clone(), q["dA"].clone()) for q in tasks]
    for q in tasks:
        q["dw"].fill_(float("nan"))
        q["dhbias"].fill_(float("nan"))
    loss2 = torch.full((1,), float("nan"), device=dev)
    ops.tower_head_fwd_bwd(ops.make_tower_head_group(tasks, prob, y, mask=mask, loss=loss2), dev, phases=True)
    assert float(loss2) == float(loss)
    for q, (w_, b_, h_, a_) in zip(tasks, keep):
        assert torch.equal(q["dw"], w_) and torch.equal(q["dhbias"], b_) and torch.equal(q["dH"], h_) and torch.equal(q["dA"], a_)


def test_tower_head_against_the_three_launches_with_regression_heads(env):
    from test_tower_head_gpu import build
    torch, L, ops, lib = env
    dev = torch.device("cuda:0")
    M, K, N, T = 16384, 128, 64, 3
    kinds = [(SIG, BCE), (IDN, MSE), (IDN, MAE)]
    y, mask, tasks = build(torch, L, ops, M, K, N, T, True, seed=5)
    gen = torch.Generator(device="cpu").manual_seed(11)
    y[:, 1] = (torch.randn(M, generator=gen) * 1.5).to(dev)
    # the MAE head's labels: float64 prediction +- (0.05 + u) -- both forms see pm on the same side of y
    pm2 = tower_reference(torch, y * 0, mask, tasks[2], 2, (IDN, MSE))[0]
    s = (torch.rand(M, generator=gen) < 0.5).double().to(dev) * 2 - 1
    y[:, 2] = (pm2 + s * (0.05 + torch.rand(M, generator=gen).double().to(dev))).float()
    for t, q in enumerate(tasks):
        q["kind"] = L.head_kind(*kinds[t])
    prob = torch.empty(M, T, device=dev)
    loss = torch.zeros(1, device=dev)
    ops.tower_head_fwd_bwd(ops.make_tower_head_group(tasks, prob, y, mask=mask, loss=loss), dev)
    hs = [torch.empty(M, N, device=dev) for _ in tasks]
    ops.gemm_fwd([dict(A=q["A"], W=q["W"], bias=q["bias1"], C=h_, act=L.ACT_RELU, amax_a=q["amax_a"], amax_w=q["amax_w"],
                       w_planes=q["planes_fwd"], w_kexp=q["kexp_fwd"]) for q, h_ in zip(tasks, hs)])
    prob2, loss2 = torch.empty(M, T, device=dev), torch.zeros(1, device=dev)
    heads = [dict(Hin=h_, w=q["w"], bias=q["hbias"], dH=torch.empty(M, N, device=dev), dw=torch.empty(N, device=dev),
                  dbias=torch.empty(1, device=dev), h_relu=1, mask_col=q["mask_col"], kind=q["kind"])
             for q, h_ in zip(tasks, hs)]
    ops.head_bce_fwd_bwd(ops.make_head_group(heads, prob2, y=y, mask=mask, loss=loss2), dev)
    # (test_tower_head_gpu.py holds probabilities to 1e-6 absolute; a raw value is held to the same distance relative to
    # the largest one)
    assert float((prob - prob2).abs().max()) < 1e-6 * max(1.0, float(prob2.abs().max()))
    assert abs(float(loss) - float(loss2)) / float(loss2) < 1e-5
    for q, hd in zip(tasks, heads):
        assert rel(q["dH"], hd["dH"].double()) < 1e-5
        assert rel(q["dw"], hd["dw"].double()) < 1e-5
        ref = hd["dH"].double() @ q["W"].double()
        assert rel(q["dA"], ref) < 1e-5


# ------------------------------------------------------------------------------------------------ ABI behaviour
def test_identity_with_bce_is_rejected(env):
    from test_tower_head_gpu import build
    torch, L, ops, lib = env
    dev = torch.device("cuda:0")
    bad = L.head_kind(L.HEAD_OUT_IDENTITY, L.HEAD_LOSS_BCE)
    for H in (64, 50):  # the fast and the general row kernel
        mask, heads, gen = build_heads(torch, L, 64, H, 2, False, False, 1, [(SIG, BCE), (IDN, MSE)], seed=H)
        heads[1]["kind"] = bad
        fresh_outputs(torch, heads, 64)
        prob, y = torch.empty(64, 2, device=dev), torch.zeros(64, 2, device=dev)
        with pytest.raises(L.MMLError) as e:
            ops.head_bce_fwd_bwd(ops.make_head_group(heads, prob, y=y, loss=torch.zeros(1, device=dev)), dev)
        assert "identity" in str(e.value)
        # without labels only the output form is read: forward and the dprob path accept it
        ops.head_fwd(ops.make_head_group(heads, prob))
        ops.head_bce_fwd_bwd(ops.make_head_group(heads, prob, dprob=torch.ones(64, 2, device=dev)), dev)
        heads[1]["kind"] = 7 << 8  # not a loss
        with pytest.raises(L.MMLError):
            ops.head_fwd(ops.make_head_group(heads, prob))
    y, mask, tasks = build(torch, L, ops, 256, 128, 64, 2, False, seed=1)
    tasks[1]["kind"] = bad
    grp = ops.make_tower_head_group(tasks, torch.empty(256, 2, device=dev), y)
    assert lib.mml_tower_head_serves(grp) == 0
    with pytest.raises(L.MMLError) as e:
        ops.tower_head_fwd_bwd(grp, dev)
    assert "identity" in str(e.value)
    torch.cuda.synchronize()


@pytest.mark.parametrize("H,gated", [(64, False), (128, True), (50, False)])
def test_zero_kinds_are_the_group_without_the_key(env, H, gated):
    torch, L, ops, lib = env
    dev = torch.device("cuda:0")
    B, T = 4099, 3
    mask, heads, gen = build_heads(torch, L, B, H, T, True, gated, 1, [(SIG, BCE)] * T, seed=H)
    y = (torch.rand(B, T, generator=gen) < 0.4).float().to(dev)
    res = []
    for with_key in (True, False):
        hs = [dict(q) for q in heads]
        for q in hs:
            if with_key:
                q["kind"] = 0
            else:
                q.pop("kind")
        fresh_outputs(torch, hs, B)
        prob, loss = torch.empty(B, T, device=dev), torch.zeros(1, device=dev)
        ops.head_bce_fwd_bwd(ops.make_head_group(hs, prob, y=y, mask=mask, loss=loss), dev)
        torch.cuda.synchronize()
        res.append((prob, loss, hs))
    (p1, l1, h1), (p2, l2, h2) = res
    assert torch.equal(p1, p2) and torch.equal(l1, l2)
    for a, b in zip(h1, h2):
        for k in ("dH", "dw", "dbias") + (("dgate",) if a.get("gate") is not None else ()):
            assert torch.equal(a[k], b[k]), k


def test_zero_kinds_tower_head_is_the_group_without_the_key(env):
    from test_tower_head_gpu import build
    torch, L, ops, lib = env
    dev = torch.device("cuda:0")
    M, T = 4099, 2
    y, mask, tasks = build(torch, L, ops, M, 128, 64, T, True, seed=3)
    outs = []
    for with_key in (True, False):
        for q in tasks:
            q.pop("kind", None)
            if with_key:
                q["kind"] = 0
            for k in ("dH", "dA", "dw", "dhbias"):
                q[k].fill_(float("nan"))
        prob, loss = torch.empty(M, T, device=dev), torch.zeros(1, device=dev)
        ops.tower_head_fwd_bwd(ops.make_tower_head_group(tasks, prob, y, mask=mask, loss=loss), dev)
        torch.cuda.synchronize()
        outs.append([prob, loss] + [q[k].clone() for q in tasks for k in ("dH", "dA", "dw", "dhbias")])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
