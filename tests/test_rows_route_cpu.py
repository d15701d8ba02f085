"""The dispatch rule of the gate and head row kernels (csrc/rows_route.hpp: family, template arguments, grid, dynamic LDS,
slab layout, workspace, refusals) off the GPU.  tests/rows_route_driver.cpp, a stand-alone program around the header, is
compiled with g++ and fed groups; every expected plan below is worked out by hand from the rule as it stood inside
csrc/rows_fast.hip and csrc/gate_head.hip before it moved, under the default switches unless the case says otherwise.
Every gate group goes through both directions, and each time the workspace the plan needs is held against what
mml_gate_mix_bwd_workspace_bytes returns and the shape-only stage (gate_rows_shape) against the plans where the group
meets its assumptions.  GATE_SYMBOLS / HEAD_SYMBOLS at the end are the (shape -> symbol) pairs that the device tests
(test_kernels_gpu.py, test_gemm16_gpu.py) read back from mml_rows_last_kernel()."""
import functools
import itertools
import os
import subprocess
import tempfile

from conftest import ROOT

ENV = dict(pack=1, fwd_mode=-1, bwd_mode=-1, hv=1, fwd_wgs="unset", bwd_wgs=4, head_wgs=2)
ERR_ARG, ERR_UNSUPPORTED = -1, -3
MIX16, DE16, DG16, E16 = 1, 2, 4, 8  # mml_gate_group.out_bf16
FAST_FWD, FAST_BWD, HV_FWD, HV_BWD = 1, 2, 4, 8  # gate_rows_shape
_tmp = None
_ptr = itertools.count(1)


def P():
    """A fresh non-null pointer, 256-byte aligned."""
    return next(_ptr) << 20


@functools.lru_cache(maxsize=None)
def driver():
    """The compiled driver (once per session, in a temporary directory that lives as long as the process)."""
    global _tmp
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import build
    _tmp = tempfile.TemporaryDirectory()
    exe = os.path.join(_tmp.name, "rows_route_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", build.CSRC,
                           os.path.join(ROOT, "tests", "rows_route_driver.cpp"), "-o", exe])
    return exe


def _drive(text, **knobs):
    k = dict(ENV, **knobs)
    head = " ".join(str(k[x]) for x in "pack fwd_mode bwd_mode hv fwd_wgs bwd_wgs head_wgs".split())
    lines = subprocess.run([driver()], input=head + " " + text + "\n", capture_output=True, text=True,
                           check=True).stdout.splitlines()
    w = lines[0].split()
    w = w[1:] if w[0] == "plan" else w
    plan = {a: (b if a in ("family", "wg_off") else int(b)) for a, b in zip(w[0::2], w[1::2])}
    if len(lines) == 1:
        return plan, None
    e = lines[1].split(" ", 2)
    return plan, "ok" if e[0] == "ok" else (int(e[1]), e[2])


# ---- gate groups as the driver reads them -----------------------------------------------------------------------------
def gates(B, H, n_experts, sets, Gd, out_bf16=0):
    """`sets`: a number of gates over all experts in order, or the expert lists; Gd: one width or one per gate."""
    sets = [list(range(n_experts))] * sets if isinstance(sets, int) else sets
    Gd = [Gd] * len(sets) if isinstance(Gd, int) else Gd
    return dict(B=B, H=H, out_bf16=out_bf16, E=[dict(E=P(), dE=P(), lde=H, ldde=H) for _ in range(n_experts)],
                gate=[dict(G=P(), Wg=P(), mix=P(), dmix=P(), dG=P(), ldg=g, ldmix=H, lddmix=H, lddg=g, Gd=g, ne=len(s),
                           active=1, expert=s) for s, g in zip(sets, Gd)])


def gate_symbol(p):
    tf = ("false", "true")
    return {"fwd_once": "gate_fwd_once_kernel<%d, %d, %d, %s, %d>" % (p["lps"], p["ne"], p["ng"], tf[p["pack"]], p["hv"]),
            "fwd_fast": "gate_fwd_fast_kernel<%d, %d>" % (p["lps"], p["ne"]),
            "bwd_fast": "gate_bwd_fast_kernel<%d, %d, %d, %d, %d>" % (p["lps"], p["ne"], p["ng"], p["mode"], p["hv"]),
            "fwd_generic": "gate_mix_fwd_kernel", "bwd_generic": "gate_mix_bwd_kernel"}[p["family"]]


def gate(g, bwd, **knobs):
    text = "gate %d %d %d %d %d %d" % (bwd, g["B"], g["H"], len(g["E"]), len(g["gate"]), g["out_bf16"])
    for x in g["E"]:
        text += " %d %d %d %d" % (x["E"], x["dE"], x["lde"], x["ldde"])
    for q in g["gate"]:
        text += "".join(" %d" % q[k] for k in "G Wg mix dmix dG ldg ldmix lddmix lddg Gd ne active".split())
        text += "".join(" %d" % e for e in q["expert"])
    p, end = _drive(text, **knobs)
    p["symbol"] = gate_symbol(p)
    return p, end


def meets_shape_assumptions(g):
    n = len(g["E"])
    ptrs = [x[k] for x in g["E"] for k in ("E", "dE")] + [q[k] for q in g["gate"] for k in ("G", "Wg", "mix", "dmix", "dG")]
    lds = [x[k] for x in g["E"] for k in ("lde", "ldde")] + [q[k] for q in g["gate"] for k in ("ldg", "ldmix", "lddmix", "lddg")]
    return (all(q["expert"] == list(range(n)) and q["Gd"] == g["gate"][0]["Gd"] and q["active"] for q in g["gate"]) and
            all(p % 16 == 0 for p in ptrs) and all(ld % 8 == 0 for ld in lds))


def both(g, **knobs):
    """Forward and backward plan of one group (the ends too), with the checks every gate case gets."""
    (f, fe), (b, be) = gate(g, 0, **knobs), gate(g, 1, **knobs)
    # what mml_gate_mix_bwd_workspace_bytes returns: 2048 workgroups of every gate's weights
    ws = 256 * 8 * sum(q["ne"] * q["Gd"] for q in g["gate"]) * 4 + 256
    for p, end in ((f, fe), (b, be)):
        if end == "ok":
            assert 1 <= p["grid"] <= 2048 and p["ws"] == (p["grid"] * p["stride"] * 4 if p is b else 0) and p["ws"] <= ws, p
            assert p["ws_first"] <= ws
    if meets_shape_assumptions(g):
        bits = ((FAST_FWD if f["family"] in ("fwd_once", "fwd_fast") else 0) | (FAST_BWD if b["family"] == "bwd_fast" else 0) |
                (HV_FWD if f["hv"] == 2 else 0) | (HV_BWD if b["hv"] == 2 else 0))
        assert f["shape"] == b["shape"] == bits, (f, b)
    return f, fe, b, be


def once_lds(lps, ng, ne, wg_total):
    return (wg_total + 4 * (64 // lps) * ng * 16 + ng * ne) * 4


def bwd_lds(lps, ng, ne, wg_total):
    spw = 64 // lps
    return (wg_total + 4 * spw * ng * 16 + 4 * spw * wg_total + ng * ne) * 4


# ---- 1, 2: the eight (NE, NG) arms, the backward's MODE ------------------------------------------------------------------
ARMS = [(4, 2, 4, 2), (4, 3, 4, 3), (4, 4, 3, 4), (4, 8, 4, 8), (4, 8, 2, 5), (8, 2, 8, 2), (8, 2, 5, 1), (8, 3, 8, 3),
        (8, 4, 6, 4), (16, 2, 16, 2), (16, 2, 9, 2)]  # NE, NG <- experts, gates (each gate over all experts)


def test_every_arm_on_every_lane_width():
    for (H, lps), (NE, NG, nexp, ngates) in itertools.product(((32, 16), (64, 16), (128, 32), (256, 64)), ARMS):
        f, fe, b, be = both(gates(1000, H, nexp, ngates, 16))
        tot = nexp * ngates * 16
        pack = "true" if (NE, NG) == (4, 2) else "false"
        mode = 1 if NE * NG <= 8 else 2
        assert fe == be == "ok"
        assert f["symbol"] == "gate_fwd_once_kernel<%d, %d, %d, %s, 1>" % (lps, NE, NG, pack), f
        assert b["symbol"] == "gate_bwd_fast_kernel<%d, %d, %d, %d, 1>" % (lps, NE, NG, mode), b
        grid = -(-1000 // (4 * 64 // lps))  # 63, 125, 250: below every cap
        assert (f["grid"], f["block"], f["lds"]) == (grid, 256, once_lds(lps, NG, NE, tot)), f
        assert (b["grid"], b["block"], b["lds"]) == (grid, 256, bwd_lds(lps, NG, NE, tot)), b
        offs = ",".join(str(i * nexp * 16) for i in range(ngates))
        assert f["wg_off"] == b["wg_off"] == offs and f["wg_total"] == b["wg_total"] == b["stride"] == tot
        assert f["ident"] == b["ident"] == 1 and b["ws"] == b["ws_first"] == grid * tot * 4


def test_flagship_plans_in_numbers():
    # AE-30's MMoE: 4 experts x 2 gates, H = 128, gate inputs of 64 columns, B = 65 536
    f, fe, b, be = both(gates(65536, 128, 4, 2, 64))
    assert (f["symbol"], f["grid"], f["lds"]) == ("gate_fwd_once_kernel<32, 4, 2, true, 1>", 1024, 3104)
    assert (b["symbol"], b["grid"], b["lds"], b["ws"]) == ("gate_bwd_fast_kernel<32, 4, 2, 1, 1>", 1024, 19488, 1024 * 512 * 4)
    # a PLE level: 8 experts x 3 gates (two over five experts, one over all), H = 128: three workgroups per CU forward
    f, fe, b, be = both(gates(65536, 128, 8, [[0, 1, 2, 6, 7], [3, 4, 5, 6, 7], list(range(8))], 64))
    assert (f["symbol"], f["grid"], f["lds"], f["wg_off"]) == ("gate_fwd_once_kernel<32, 8, 3, false, 1>", 768, 6240, "0,320,640")
    assert (b["symbol"], b["grid"], b["lds"], b["ident"]) == ("gate_bwd_fast_kernel<32, 8, 3, 2, 1>", 1024, 43104, 0)


def test_backward_mode():
    # identity maps and ne * ng <= 8: every expert row loaded once and kept
    assert both(gates(1000, 64, 4, 2, 16))[2]["mode"] == 1 and both(gates(1000, 64, 3, 1, 16))[2]["mode"] == 1
    # more than eight coefficients, or maps that are not the identity: one load per gate pass
    assert both(gates(1000, 64, 4, 3, 16))[2]["mode"] == 2
    assert both(gates(1000, 64, 4, [[0, 1, 2, 3], [3, 1]], 16))[2]["mode"] == 2
    assert both(gates(1000, 64, 3, [[2, 0, 1]], 16))[2]["symbol"] == "gate_bwd_fast_kernel<16, 4, 2, 2, 1>"
    # more experts than a gate mixes (two gates over disjoint halves of eight): per gate and expert, both directions
    f, fe, b, be = both(gates(1000, 32, 8, [[0, 1, 2, 3], [4, 5, 6, 7]], 16))
    assert (f["symbol"], f["lds"]) == ("gate_fwd_fast_kernel<16, 4>", 128 * 4)
    assert (b["symbol"], b["lds"]) == ("gate_bwd_fast_kernel<16, 4, 2, 0, 1>", (128 + 512 + 16 * 128 + 8) * 4)
    # MMLREC_GATE_BWD_MODE: 0 everywhere; 2 where 1 would run; 1 cannot be had where it does not apply
    g = gates(1000, 64, 4, 2, 16)
    assert [both(g, bwd_mode=m)[2]["mode"] for m in (0, 1, 2)] == [0, 1, 2]
    assert [both(gates(1000, 64, 8, 2, 16), bwd_mode=m)[2]["mode"] for m in (0, 1, 2)] == [0, 2, 2]
    # MMLREC_GATE_FWD_MODE=0: the per-gate forward everywhere
    assert both(g, fwd_mode=0)[0]["symbol"] == "gate_fwd_fast_kernel<16, 4>"
    assert both(gates(1000, 128, 8, 3, 16), fwd_mode=0)[0]["symbol"] == "gate_fwd_fast_kernel<32, 8>"
    # MMLREC_GATE_PACK=0: the eight separate butterflies
    assert both(g, pack=0)[0]["symbol"] == "gate_fwd_once_kernel<16, 4, 2, false, 1>"


# ---- 3: more than 32 coefficients -------------------------------------------------------------------------------------------
def test_register_budget():
    for nexp, ngates, NE in ((16, 3, 16), (8, 8, 8), (9, 3, 16)):
        f, fe, b, be = both(gates(70, 32, nexp, ngates, 16))
        tot = nexp * ngates * 16
        assert (f["symbol"], f["grid"], f["lds"], fe) == ("gate_fwd_fast_kernel<16, %d>" % NE, 5, tot * 4, "ok")
        assert (b["symbol"], b["grid"], b["block"], b["lds"], be) == ("gate_mix_bwd_kernel", 18, 256, (tot + 512) * 4, "ok")
        assert (b["ws"], b["ws_first"], b["stride"]) == (18 * tot * 4, 0, tot)
    # (the forward's three workgroups per CU hold for the per-gate kernel too)
    assert both(gates(10 ** 6, 32, 16, 3, 16))[0]["grid"] == 768


# ---- 4, 5: the generic family and its refusals ---------------------------------------------------------------------------
def _generic_cases():
    g = gates(1000, 30, 4, 2, 16)
    yield "H % 4", g, True, True
    yield "H > 256", gates(1000, 300, 3, [[2, 0]], 100), True, True
    yield "Gd > 256", gates(1000, 64, 4, 2, 260), True, True
    g = gates(1000, 64, 4, 2, 16)
    g["E"][1]["E"] += 4
    yield "misaligned expert", g, True, True
    g = gates(1000, 64, 4, 2, 16)
    g["gate"][1]["Wg"] += 8
    yield "misaligned gate weight", g, True, True
    g = gates(1000, 64, 4, 2, 16)
    g["E"][2]["lde"] = 66
    yield "pitch 4k + 2", g, True, True
    g = gates(1000, 64, 4, 2, 16)
    g["gate"][0]["ldmix"] = 70  # (the forward's own buffer: the backward does not read it)
    yield "mix pitch 4k + 2", g, True, False
    g = gates(1000, 64, 4, 2, 16)
    g["gate"][0]["lddg"] = 18
    yield "dG pitch 4k + 2", g, False, True


def test_generic_family():
    for what, g, fwd_generic, bwd_generic in _generic_cases():
        f, fe, b, be = both(g)
        tot = sum(q["ne"] * q["Gd"] for q in g["gate"])
        assert fe == be == "ok", what
        assert (f["family"] == "fwd_generic", b["family"] == "bwd_generic") == (fwd_generic, bwd_generic), what
        if fwd_generic:
            assert (f["symbol"], f["grid"], f["block"], f["lds"]) == ("gate_mix_fwd_kernel", 250, 256, 0), what
        if bwd_generic:
            assert (b["symbol"], b["grid"], b["block"], b["lds"]) == ("gate_mix_bwd_kernel", 250, 256, (tot + 512) * 4), what
            assert (b["ws"], b["ws_first"], b["stride"], b["wg_total"]) == (250 * tot * 4, 0, tot, tot), what
        # bf16 outputs exist in the fast kernels only
        g["out_bf16"] = MIX16 | DE16
        f, fe, b, be = both(g)
        if fwd_generic:
            assert fe == (ERR_UNSUPPORTED, "mml_gate_mix_fwd: out_bf16 on a shape the fast row kernel does not serve"), what
        if bwd_generic:
            assert be == (ERR_UNSUPPORTED, "mml_gate_mix_bwd: out_bf16 on a shape the fast row kernel does not serve"), what


def test_generic_backward_keeps_active_gates_only():
    g = gates(515, 300, 8, [[0, 1, 2, 6, 7], [3, 4, 5, 6, 7], list(range(8))], 16)
    g["gate"][1]["active"] = 0
    b = both(g)[2]
    assert (b["wg_off"], b["wg_total"], b["grid"], b["ws"]) == ("0,80,80", 208, 129, 129 * 208 * 4)
    # the fast kernels lay out every gate
    g = gates(515, 32, 8, [[0, 1, 2, 6, 7], [3, 4, 5, 6, 7], list(range(8))], 16)
    g["gate"][2]["active"] = 0
    b = both(g)[2]
    assert (b["symbol"], b["wg_off"], b["wg_total"]) == ("gate_bwd_fast_kernel<16, 8, 3, 2, 1>", "0,80,160", 288)


def test_lds_budgets():
    # forward: gate weights of more than 48 KiB -> generic; this group's backward (64 coefficients) is generic anyway and
    # its accumulators do not fit 64 KiB
    g = gates(1000, 256, 8, 8, 256)
    f, fe, b, be = both(g)
    assert (f["symbol"], f["grid"], fe) == ("gate_mix_fwd_kernel", 250, "ok")
    assert be == (ERR_ARG, "mml_gate_mix_bwd: gate weights too large for the LDS accumulators (67584 B)")
    assert (b["ws"], b["ws_first"]) == (250 * 16384 * 4, 0)
    g["out_bf16"] = MIX16
    f, fe, b, be = both(g)
    assert fe[0] == be[0] == ERR_UNSUPPORTED
    # 12 288 floats of gate weights are the last that fit the per-gate forward (the load-once form stops earlier)
    assert both(gates(1000, 256, 16, 3, 256))[0]["symbol"] == "gate_fwd_fast_kernel<64, 16>"
    assert both(gates(1000, 256, 16, [list(range(16))] * 3 + [[0]], [256, 256, 256, 4]))[0]["symbol"] == "gate_mix_fwd_kernel"
    # load-once forward: 60 KiB with the probabilities and the maps (under 48 KiB of weights they always fit)
    assert both(gates(1000, 256, 8, 4, 256))[0]["symbol"] == "gate_fwd_once_kernel<64, 8, 4, false, 1>"  # 8192 floats
    assert both(gates(1000, 256, 16, 2, 256))[0]["lds"] == (8192 + 128 + 32) * 4
    f = both(gates(1000, 64, 4, 8, 256))[0]  # the largest: 8192 floats of weights + 512 + 32 more
    assert (f["symbol"], f["lds"]) == ("gate_fwd_once_kernel<64, 4, 8, false, 1>", 34944)
    # fast backward over 60 KiB: the generic kernel, but the workspace is asked for as the fast kernel would use it first
    f, fe, b, be = both(gates(1000, 128, 8, 4, 128))  # 32-lane groups: (4096 + 512 + 8 * 4096 + 32) * 4 = 149 632 B
    assert (b["symbol"], b["grid"], b["lds"], be) == ("gate_mix_bwd_kernel", 250, (4096 + 512) * 4, "ok")
    assert (b["ws_first"], b["ws"]) == (125 * 4096 * 4, 250 * 4096 * 4)
    g = gates(1000, 128, 8, 4, 128, out_bf16=DE16 | DG16)
    b, be = both(g)[2:]
    assert be == (ERR_UNSUPPORTED, "mml_gate_mix_bwd: out_bf16 on a shape the fast row kernel does not serve")
    assert b["ws_first"] == 125 * 4096 * 4
    # the largest that fits: 4 x 2 on 64-lane groups with 256-wide gate inputs
    assert both(gates(1000, 256, 4, 2, 256))[2]["lds"] == (2048 + 128 + 4 * 2048 + 8) * 4


# ---- 6: eight row columns per lane (HV = 2) --------------------------------------------------------------------------------
HV_F, HV_B = "gate_fwd_once_kernel<32, 4, 2, true, 2>", "gate_bwd_fast_kernel<32, 4, 2, 1, 2>"
W_F, W_B = "gate_fwd_once_kernel<64, 4, 2, true, 1>", "gate_bwd_fast_kernel<64, 4, 2, 1, 1>"


def syms(g, **knobs):
    f, fe, b, be = both(g, **knobs)
    assert fe == be == "ok"
    return f["symbol"], b["symbol"]


def test_hv_form():
    for H, nexp, ngates in ((256, 4, 2), (136, 4, 2), (192, 3, 1)):
        g = gates(1000, H, nexp, ngates, 128, out_bf16=E16 | MIX16 | DE16)
        f, fe, b, be = both(g)
        tot = nexp * ngates * 128
        assert (f["symbol"], f["grid"], f["lds"]) == (HV_F, 125, once_lds(32, 2, 4, tot))
        assert (b["symbol"], b["grid"], b["lds"]) == (HV_B, 125, bwd_lds(32, 2, 4, tot))
    g = gates(1000, 256, 4, 2, 128, out_bf16=E16)
    assert both(g)[0]["lds"] == 5152 and both(g)[2]["lds"] == 37920
    # not without bf16 experts, not for rows of at most 128 columns, not for H % 8 != 0, not for wider gate inputs, not for
    # more gates or experts
    assert syms(gates(1000, 256, 4, 2, 128)) == (W_F, W_B)
    assert syms(gates(1000, 128, 4, 2, 128, out_bf16=E16)) == ("gate_fwd_once_kernel<32, 4, 2, true, 1>",
                                                                "gate_bwd_fast_kernel<32, 4, 2, 1, 1>")
    assert syms(gates(1000, 252, 4, 2, 128, out_bf16=E16)) == (W_F, W_B)
    assert syms(gates(1000, 256, 4, 2, 132, out_bf16=E16)) == (W_F, W_B)
    assert syms(gates(1000, 256, 4, 2, [128, 132], out_bf16=E16)) == (W_F, W_B)
    assert syms(gates(1000, 256, 4, 3, 128, out_bf16=E16)) == ("gate_fwd_once_kernel<64, 4, 3, false, 1>",
                                                                "gate_bwd_fast_kernel<64, 4, 3, 2, 1>")
    assert syms(gates(1000, 256, 5, 2, 128, out_bf16=E16))[0] == "gate_fwd_once_kernel<64, 8, 2, false, 1>"
    # pitches: expert rows of 8k bf16 values; dE rows of 8k when they are bf16, else 4k (backward); the same for mix (forward)
    g = gates(1000, 256, 4, 2, 128, out_bf16=E16)
    g["E"][3]["lde"] = 260
    assert syms(g) == (W_F, W_B)
    g = gates(1000, 256, 4, 2, 128, out_bf16=E16)
    g["E"][0]["ldde"], g["gate"][1]["ldmix"] = 260, 260
    assert syms(g) == (HV_F, HV_B)
    g["out_bf16"] = E16 | DE16
    assert syms(g) == (HV_F, W_B)
    g["out_bf16"] = E16 | MIX16
    assert syms(g) == (W_F, HV_B)
    # the backward's form keeps every expert row: identity maps only (the forward does not care)
    g = gates(1000, 256, 4, [[0, 1, 2, 3], [1, 0, 2, 3]], 128, out_bf16=E16)
    assert syms(g) == (HV_F, "gate_bwd_fast_kernel<64, 4, 2, 2, 1>")
    # the switches
    g = gates(1000, 256, 4, 2, 128, out_bf16=E16)
    assert syms(g, pack=0) == ("gate_fwd_once_kernel<64, 4, 2, false, 1>", W_B)
    assert syms(g, hv=0) == (W_F, W_B)
    assert syms(g, hv=2) == (HV_F, HV_B)
    assert syms(g, bwd_mode=1) == (HV_F, W_B)
    assert syms(g, bwd_mode=2) == (HV_F, "gate_bwd_fast_kernel<64, 4, 2, 2, 1>")
    assert syms(g, fwd_mode=0) == ("gate_fwd_fast_kernel<64, 4>", HV_B)


def test_hv_lab_form_on_16_lane_groups():
    # MMLREC_GATE_HV=2: fp32 rows of 65..128 columns under gate inputs of at most 64 (AE-30's MMoE)
    g = gates(1000, 128, 4, 2, 64)
    f, fe, b, be = both(g, hv=2)
    assert (f["symbol"], f["grid"], f["lds"]) == ("gate_fwd_once_kernel<16, 4, 2, true, 2>", 63, 4128)
    assert (b["symbol"], b["grid"], b["lds"]) == ("gate_bwd_fast_kernel<16, 4, 2, 1, 2>", 63, 36896)
    assert syms(g) == ("gate_fwd_once_kernel<32, 4, 2, true, 1>", "gate_bwd_fast_kernel<32, 4, 2, 1, 1>")
    for other in (gates(1000, 64, 4, 2, 64), gates(1000, 128, 4, 2, 68), gates(1000, 128, 4, 2, 64, out_bf16=E16),
                  gates(1000, 132, 4, 2, 64)):
        assert all(", 1>" in s for s in syms(other, hv=2))


# ---- 7: grids ------------------------------------------------------------------------------------------------------------------
def test_gate_grids():
    def grids(g, **knobs):
        f, fe, b, be = both(g, **knobs)
        return f["grid"], b["grid"]
    for B, n in ((1, 1), (16, 1), (17, 2), (16 * 40 + 1, 41), (10 ** 6, 1024)):  # 16 samples per workgroup; 4 per CU
        assert grids(gates(B, 64, 4, 2, 16)) == (n, n)
    assert grids(gates(1001, 256, 4, 2, 16)) == (251, 251)  # 64-lane groups: 4 samples per workgroup
    # more than 16 coefficients: three per CU forward -- unless MMLREC_GATE_FWD_WGS says otherwise, for every group
    assert grids(gates(10 ** 6, 64, 8, 3, 16)) == (768, 1024)
    assert grids(gates(10 ** 6, 64, 8, 2, 16)) == (1024, 1024)
    assert grids(gates(10 ** 6, 64, 8, 3, 16), fwd_wgs=6) == (1536, 1024)
    assert grids(gates(10 ** 6, 64, 4, 2, 16), fwd_wgs=6) == (1536, 1024)
    assert grids(gates(10 ** 6, 64, 8, 3, 16), fwd_wgs=4) == (1024, 1024)
    assert grids(gates(10 ** 6, 64, 4, 2, 16), bwd_wgs=2) == (1024, 512)
    assert grids(gates(10 ** 6, 64, 4, 2, 16), bwd_wgs=8, fwd_wgs=1) == (256, 2048)
    assert grids(gates(10 ** 6, 64, 4, 2, 16), fwd_wgs=0) == (1, 1024)
    # the generic kernels: one sample per wave, eight workgroups per CU
    assert grids(gates(10 ** 6, 30, 4, 2, 16)) == (2048, 2048) and grids(gates(1, 30, 4, 2, 16)) == (1, 1)
    assert grids(gates(4 * 77 + 1, 30, 4, 2, 16)) == (78, 78)


# ---- 8: heads ------------------------------------------------------------------------------------------------------------------
KIND_IDENT_MSE, KIND_IDENT_MAE = (1 << 8) | 1, (2 << 8) | 1  # MML_HEAD_KIND(identity, MSE / MAE)


def heads(B, Hs, gated=(), kinds=None, dh_bf16=0):
    kinds = kinds or [0] * len(Hs)
    return dict(B=B, dh_bf16=dh_bf16,
                head=[dict(Hin=P(), w=P(), w2=0, dH=P(), gate=P() if t in gated else 0, dgate=P() if t in gated else 0, ldh=H,
                           lddh=H, ldgate=H, lddgate=H, H=H, kind=kinds[t]) for t, H in enumerate(Hs)])


def head(g, train, **knobs):
    text = "head %d %d %d %d" % (train, g["B"], len(g["head"]), g["dh_bf16"])
    for q in g["head"]:
        text += "".join(" %d" % q[k] for k in "Hin w w2 dH gate dgate ldh lddh ldgate lddgate H kind".split())
    p, end = _drive(text, **knobs)
    tf = ("false", "true")
    p["symbol"] = ("head_fast_kernel<%d, %d, %s, %s>" % (p["lps"], p["nt"], tf[p["gated"]], tf[p["kinds"]])
                   if p["family"] == "fast" else "head_kernel<%s>" % tf[p["kinds"]])
    # what mml_head_workspace_bytes returns: 2048 workgroups
    ws = 256 * 8 * (len(g["head"]) * (p["hmax"] + 1) + 1) * 4 + 256
    assert 1 <= p["grid"] <= 2048 and p["ws"] == p["grid"] * p["stride"] * 4 <= ws, p
    assert p["stride"] == (len(g["head"]) * (p["hmax"] + 1) + 1 if train else 0)
    return p, end


def test_head_plans():
    for n, NT in ((1, 2), (2, 2), (3, 4), (4, 4), (5, 8), (8, 8)):
        for H, lps in ((16, 16), (64, 16), (68, 32), (128, 32), (200, 64), (256, 64)):
            for train in (0, 1):
                p, end = head(heads(1000, [H] * n), train)
                grid = -(-1000 // (4 * 64 // lps))
                assert (p["symbol"], p["grid"], p["block"], p["hmax"], end) == (
                    "head_fast_kernel<%d, %d, false, false>" % (lps, NT), grid, 256, H, "ok")
    # the widest head picks the lane groups; gated, kinds
    p, end = head(heads(1000, [16, 128, 64], gated=(1,)), 1)
    assert (p["symbol"], p["hmax"], p["stride"], p["ws"]) == ("head_fast_kernel<32, 4, true, false>", 128, 388, 125 * 388 * 4)
    p, end = head(heads(1000, [64, 64], kinds=[0, KIND_IDENT_MSE]), 0)
    assert (p["symbol"], p["out_bits"], p["loss_bits"], p["stride"]) == ("head_fast_kernel<16, 2, false, true>", 2, 4, 0)
    p, end = head(heads(1000, [64] * 4, gated=(0, 1, 2, 3), kinds=[KIND_IDENT_MAE, 0, KIND_IDENT_MSE, 1]), 1)
    assert (p["symbol"], p["out_bits"], p["loss_bits"]) == ("head_fast_kernel<16, 4, true, true>", 0b1101, 0b00010010)
    # bf16 dH: the fast kernel's, plain heads only
    assert head(heads(1000, [64, 64], dh_bf16=1), 1)[0]["symbol"] == "head_fast_kernel<16, 2, false, false>"


def test_head_grids():
    assert [head(heads(B, [64, 64]), 1)[0]["grid"] for B in (1, 16, 17, 10 ** 6)] == [1, 1, 2, 512]
    assert head(heads(10 ** 6, [64, 64]), 1, head_wgs=8)[0]["grid"] == 2048
    assert head(heads(10 ** 6, [64, 64]), 0, head_wgs=1)[0]["grid"] == 256
    assert head(heads(10 ** 6, [200, 64]), 0)[0]["grid"] == 512 and head(heads(1001, [200, 64]), 0)[0]["grid"] == 251


def test_head_generic_family_and_refusals():
    cases = [heads(1000, [30, 64]), heads(1000, [64, 62])]
    g = heads(1000, [64, 64])
    g["head"][1]["Hin"] += 4
    cases.append(g)
    g = heads(1000, [64, 64])
    g["head"][0]["ldh"] = 66
    cases.append(g)
    g = heads(1000, [64, 64])
    g["head"][0]["w2"] = P() + 4
    cases.append(g)
    for g in cases:
        for train in (0, 1):
            p, end = head(g, train)
            assert (p["symbol"], p["grid"], p["block"], p["hmax"], end) == ("head_kernel<false>", 250, 256, 64, "ok")
            assert p["stride"] == (2 * 65 + 1 if train else 0)
        g["head"][1]["kind"] = KIND_IDENT_MSE
        assert head(g, 1)[0]["symbol"] == "head_kernel<true>"
    g = heads(1000, [64, 64])
    g["head"][0]["lddh"] = 66  # (the backward's own buffer)
    assert head(g, 0)[0]["family"] == "fast" and head(g, 1)[0]["family"] == "generic"
    assert head(heads(10 ** 6, [30]), 1)[0]["grid"] == 2048
    # gated heads and bf16 dH exist in the fast kernel only
    fwd_msg = "mml_head_fwd: gated heads on a shape the fast row kernel does not serve"
    train_msg = "mml_head_bce_fwd_bwd: dh_bf16 / gated heads on a shape the fast row kernel does not serve"
    g = heads(1000, [30, 64], gated=(1,))
    assert head(g, 0)[1] == (ERR_UNSUPPORTED, fwd_msg) and head(g, 1)[1] == (ERR_UNSUPPORTED, train_msg)
    g = heads(1000, [30, 64], dh_bf16=1)
    assert head(g, 0)[1] == "ok" and head(g, 1)[1] == (ERR_UNSUPPORTED, train_msg)
    g = heads(1000, [64, 64], gated=(0,), dh_bf16=1)  # (a gated head's dH is fp32)
    assert head(g, 0)[1] == (ERR_UNSUPPORTED, fwd_msg) and head(g, 1)[1] == (ERR_UNSUPPORTED, train_msg)
    g = heads(1000, [64, 64], gated=(0,))
    g["head"][0]["lddgate"] = 66
    assert head(g, 0)[1] == "ok" and head(g, 1)[1] == (ERR_UNSUPPORTED, train_msg)
    p, end = head(g, 1)  # the refused group's layout is the generic kernel's (the reduction phase alone still finds it)
    assert (p["family"], p["grid"], p["stride"]) == ("generic", 250, 131)


# ---- 10, 11: the shape-only stage and what model/mmoe.py makes of it ------------------------------------------------------
def shape(H, gd, ne, ng, e16, **knobs):
    return _drive("shape %d %d %d %d %d" % (H, gd, ne, ng, e16), **knobs)[0]["shape"]


def test_shape_stage():
    assert shape(128, 64, 4, 2, 0) == FAST_FWD | FAST_BWD
    assert shape(256, 128, 4, 2, 1) == FAST_FWD | FAST_BWD | HV_FWD | HV_BWD
    assert shape(256, 128, 4, 2, 1, pack=0) == shape(256, 128, 4, 2, 1, hv=0) == FAST_FWD | FAST_BWD
    assert shape(256, 128, 4, 2, 1, fwd_mode=0) == FAST_FWD | FAST_BWD | HV_BWD
    assert shape(256, 128, 4, 2, 1, bwd_mode=1) == FAST_FWD | FAST_BWD | HV_FWD
    assert shape(128, 64, 4, 2, 0, hv=2) == FAST_FWD | FAST_BWD | HV_FWD | HV_BWD
    assert shape(32, 16, 16, 3, 0) == shape(32, 16, 8, 8, 0) == FAST_FWD  # more than 32 coefficients
    assert shape(128, 128, 8, 4, 0) == FAST_FWD                            # fast backward over 60 KiB
    assert shape(256, 256, 8, 8, 0) == 0                                   # gate weights over 48 KiB
    assert shape(30, 16, 4, 2, 0) == shape(300, 16, 4, 2, 0) == shape(64, 18, 4, 2, 0) == shape(64, 260, 4, 2, 0) == 0
    assert shape(64, 0, 4, 2, 0) == shape(64, 16, 0, 2, 0) == shape(64, 16, 17, 2, 0) == shape(64, 16, 4, 9, 0) == 0


def test_bf16_experts_default_follows_the_library():
    """model/mmoe.py stores the expert outputs as bf16 by default exactly where the library runs the HV = 2 kernels.  Under
    the default switches that is the expression the model used to evaluate by hand."""
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd.model import mmoe
    for H, G, Ne, T_ in itertools.product((64, 128, 132, 136, 192, 256, 260), (0, 64, 128, 130, 132), (2, 4, 5), (1, 2, 3)):
        before = 128 < H <= 256 and H % 8 == 0 and 0 < G <= 128 and G % 4 == 0 and Ne <= 4 and T_ <= 2
        for training in (False, True):
            assert mmoe.experts_bf16_by_default(H, G, Ne, T_, training) == before, (H, G, Ne, T_, training)


# ---- 12: what the device tests read back from mml_rows_last_kernel() ---------------------------------------------------
# tests/test_kernels_gpu.py::test_gate_mix_fwd_bwd: (B, H, experts, gate sets, Gd) -> (forward, backward)
ALL = lambda n, k: [list(range(n))] * k  # noqa: E731
GATE_SYMBOLS = {
    (1000, 128, 4, 2, 64): ("gate_fwd_once_kernel<32, 4, 2, true, 1>", "gate_bwd_fast_kernel<32, 4, 2, 1, 1>"),
    (515, 32, 8, 3, 16): ("gate_fwd_once_kernel<16, 8, 3, false, 1>", "gate_bwd_fast_kernel<16, 8, 3, 2, 1>"),
    (70, 300, 3, 1, 100): ("gate_mix_fwd_kernel", "gate_mix_bwd_kernel"),
    (300, 256, 4, 2, 128): ("gate_fwd_once_kernel<64, 4, 2, true, 1>", "gate_bwd_fast_kernel<64, 4, 2, 1, 1>"),
    (257, 64, 3, 1, 32): ("gate_fwd_once_kernel<16, 4, 2, true, 1>", "gate_bwd_fast_kernel<16, 4, 2, 2, 1>"),
    (129, 128, 4, 2, 64): ("gate_fwd_once_kernel<32, 4, 2, true, 1>", "gate_bwd_fast_kernel<32, 4, 2, 2, 1>"),
    (1000, 64, 4, 2, 16): ("gate_fwd_once_kernel<16, 4, 2, true, 1>", "gate_bwd_fast_kernel<16, 4, 2, 1, 1>"),
    (70, 32, 4, 3, 16): ("gate_fwd_once_kernel<16, 4, 3, false, 1>", "gate_bwd_fast_kernel<16, 4, 3, 2, 1>"),
    (70, 32, 4, 4, 16): ("gate_fwd_once_kernel<16, 4, 4, false, 1>", "gate_bwd_fast_kernel<16, 4, 4, 2, 1>"),
    (70, 32, 4, 8, 16): ("gate_fwd_once_kernel<16, 4, 8, false, 1>", "gate_bwd_fast_kernel<16, 4, 8, 2, 1>"),
    (70, 32, 8, 2, 16): ("gate_fwd_once_kernel<16, 8, 2, false, 1>", "gate_bwd_fast_kernel<16, 8, 2, 2, 1>"),
    (70, 32, 8, 4, 16): ("gate_fwd_once_kernel<16, 8, 4, false, 1>", "gate_bwd_fast_kernel<16, 8, 4, 2, 1>"),
    (70, 32, 16, 2, 16): ("gate_fwd_once_kernel<16, 16, 2, false, 1>", "gate_bwd_fast_kernel<16, 16, 2, 2, 1>"),
    (70, 32, 16, 3, 16): ("gate_fwd_fast_kernel<16, 16>", "gate_mix_bwd_kernel"),
    (70, 32, 8, 8, 16): ("gate_fwd_fast_kernel<16, 8>", "gate_mix_bwd_kernel"),
    (70, 32, 8, "halves", 16): ("gate_fwd_fast_kernel<16, 4>", "gate_bwd_fast_kernel<16, 4, 2, 0, 1>"),
}
GATE_SETS = {  # the gate sets of the cases above that are not "every gate over all experts"
    (515, 32, 8, 3, 16): [[0, 1, 2, 6, 7], [3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6, 7]],
    (70, 300, 3, 1, 100): [[2, 0]],
    (257, 64, 3, 1, 32): [[2, 0, 1]],
    (129, 128, 4, 2, 64): [[0, 1, 2, 3], [3, 1]],
    (70, 32, 8, "halves", 16): [[0, 1, 2, 3], [4, 5, 6, 7]],
}


def gate_symbols_key(B, H, nexp, gate_sets, Gd):
    """The key of GATE_SYMBOLS for a case of test_gate_mix_fwd_bwd."""
    for k, sets in GATE_SETS.items():
        if k[:3] == (B, H, nexp) and sets == gate_sets:
            return k
    assert gate_sets == ALL(nexp, len(gate_sets))
    return (B, H, nexp, len(gate_sets), Gd)


# test_head_bce / test_gated_head_bce: (H, heads, gated) -> the symbol of the training call and of the forward-only call;
# test_gemm16_gpu.py's HV test: the two HV = 2 symbols
HEAD_SYMBOLS = {
    (64, 2, False): "head_fast_kernel<16, 2, false, false>", (16, 4, False): "head_fast_kernel<16, 4, false, false>",
    (200, 1, False): "head_fast_kernel<64, 2, false, false>", (128, 4, True): "head_fast_kernel<32, 4, true, false>",
    (64, 2, True): "head_fast_kernel<16, 2, true, false>", (16, 3, True): "head_fast_kernel<16, 4, true, false>",
}
HV_SYMBOLS = (HV_F, HV_B)


def test_symbols_the_device_tests_read_back():
    for key, (fs, bs) in GATE_SYMBOLS.items():
        B, H, nexp, ngates, Gd = key
        g = gates(B, H, nexp, GATE_SETS.get(key, ngates), Gd)
        if key == (515, 32, 8, 3, 16):
            g["gate"][2]["active"] = 0  # (the device test's inactive PLE gate)
        assert syms(g) == (fs, bs), key
    for (H, n, gated), s in HEAD_SYMBOLS.items():
        g = heads(1000, [H] * n, gated=range(n - 1 if n == 3 else n) if gated else ())
        assert head(g, 1)[0]["symbol"] == head(g, 0)[0]["symbol"] == s
    # test_gate_kernels_with_eight_columns_per_lane_against_float64: 4 bf16 experts x 2 gates, bf16 and fp32 mix / dE
    for (B, H, Gd), out16 in itertools.product(((333, 200, 72), (4099, 256, 128), (64, 136, 128)), (MIX16 | DE16, 0)):
        assert syms(gates(B, H, 4, 2, Gd, out_bf16=E16 | out16)) == HV_SYMBOLS
