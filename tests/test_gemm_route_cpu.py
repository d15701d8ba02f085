"""The dispatch rule of the grouped GEMMs (csrc/gemm_route.hpp: family, template arguments, grid, dynamic LDS, refusals)
off the GPU.  tests/gemm_route_driver.cpp, a stand-alone program around the header, is compiled with g++ and fed calls;
every expected launch below is worked out by hand from the rule as it stood inside the kernels' files before it moved,
for 256 compute units and the default switches unless the case says otherwise.  The last tests (test_shapes_of_*) hold
the (shape, switches) -> symbol pairs that the device tests (test_gemm_{panel,ws,os,nt,pipe}_gpu.py, test_pep_gate_gpu.py,
test_star_linear_gpu.py) read back from mml_gemm_last_kernel(), with the literals or substrings those tests assert."""
import functools
import itertools
import os
import subprocess
import tempfile

from conftest import ROOT

RELU, NONE, SIGMOID2 = 1, 0, 3
ENV = dict(mode=4, panel=1, ws=1, os=1, nt=1, per_cu=2, glds=1, planes=1, bn=0, pad=0, cus=256)
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
    exe = os.path.join(_tmp.name, "gemm_route_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", build.CSRC,
                           os.path.join(ROOT, "tests", "gemm_route_driver.cpp"), "-o", exe])
    return exe


# ---- descriptors as the driver reads them -----------------------------------------------------------------------------
def fwd(M, K, N, act=RELU, w_kn=0, masks=False, k7=False, **over):
    d = dict(A=P(), W=P(), bias=P(), C=P(), lda=K, ldw=N if w_kn else K, ldc=N, M=M, N=N, K=K, act=act, w_kn=w_kn,
             relu_mask=P() if masks else 0, ldmask=(N + 31) // 32, amax_a=P(), amax_w=P(), amax_out=P(), w_planes=P(),
             w_kexp=P(), mul=P() if k7 else 0, prod=P() if k7 else 0, ldmul=N if k7 else 0, ldprod=N if k7 else 0,
             amax_prod=P() if k7 else 0)
    d.update(over)
    return d


FWD_KEYS = ("A W bias C lda ldw ldc M N K act w_kn relu_mask ldmask amax_a amax_w amax_out w_planes w_kexp mul prod ldmul "
            "ldprod amax_prod").split()


def dgrad(M, K, Ns, act=NONE, w_kn=0, masks=False, kexp=None, **over):
    """dA [M, K] = sum over the sources dC_s [M, N_s] W_s; one exponent word for all sources unless kexp lists them."""
    kexp = kexp or [P()] * len(Ns)
    d = dict(dA=P(), Y=0, ldda=K, ldy=0, M=M, K=K, act=RELU if masks else act, n_src=len(Ns), accumulate=0,
             relu_mask=P() if masks else 0, ldmask=(K + 31) // 32, amax_out=P(), gate_h=0, gate_g=0, d_h=0, d_g=0, ld_h=0,
             ld_g=0, ld_dh=0, ld_dg=0, act_h=0, act_g=0, acc_h=0, acc_g=0,
             src=[dict(dC=P(), W=P(), lddc=n, ldw=n if w_kn else K, N=n, w_kn=w_kn, amax_dc=P(), amax_w=P(), w_planes=P(),
                       w_kexp=kexp[s]) for s, n in enumerate(Ns)])
    d.update(over)
    return d


DGRAD_KEYS = ("dA Y ldda ldy M K act n_src accumulate relu_mask ldmask amax_out gate_h gate_g d_h d_g ld_h ld_g ld_dh ld_dg "
              "act_h act_g acc_h acc_g").split()
SRC_KEYS = "dC W lddc ldw N w_kn amax_dc amax_w w_planes w_kexp".split()


def wgrad(M, N, K, w_kn=0, **over):
    d = dict(dC=P(), A=P(), dW=P(), dbias=P(), lddc=N, lda=K, lddw=N if w_kn else K, M=M, N=N, K=K, accumulate=0, w_kn=w_kn,
             amax_dc=P(), amax_a=P())
    d.update(over)
    return d


WGRAD_KEYS = "dC A dW dbias lddc lda lddw M N K accumulate w_kn amax_dc amax_a".split()


def run(kind, descs, ws_bytes=1 << 30, phase=0, **knobs):
    """One call through the driver -> (launches, end): launches are (symbol, dict of the plan's numbers), end is "ok",
    ("refused", code, message) or ("bytes", n)."""
    k = dict(ENV, **knobs)
    text = " ".join(str(k[x]) for x in "mode panel ws os nt per_cu glds planes bn pad cus".split())
    text += " %s %d" % (kind, len(descs))
    if kind == "wgrad":
        text += " %d %d" % (ws_bytes, phase)
    for d in descs:
        if kind == "fwd":
            text += "".join(" %d" % d[x] for x in FWD_KEYS)
        elif kind == "dgrad":
            text += "".join(" %d" % d[x] for x in DGRAD_KEYS)
            for s in d["src"][:max(0, min(d["n_src"], 8))]:
                text += "".join(" %d" % s[x] for x in SRC_KEYS)
        else:
            text += "".join(" %d" % d[x] for x in WGRAD_KEYS)
    lines = subprocess.run([driver()], input=text + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    launches = []
    for ln in lines[:-1]:
        assert ln.startswith("launch "), lines
        sym, rest = ln[len("launch "):].split(" | ")
        w = rest.split()
        launches.append((sym, {a: (b if a == "members" else int(b)) for a, b in zip(w[0::2], w[1::2])}))
    w = lines[-1].split(" ", 2)
    end = "ok" if w[0] == "ok" else (w[0], int(w[1])) + tuple(w[2:])
    return launches, end


def one(kind, descs, **kw):
    """The call's only launch as (symbol, grid, dynamic LDS, the plan's numbers)."""
    launches, end = run(kind, descs, **kw)
    assert end == "ok" and len(launches) == 1, (launches, end)
    sym, f = launches[0]
    return sym, f["grid"], f["dyn"], f


def brief(kind, descs, **kw):
    return one(kind, descs, **kw)[:2]


# ---- gemm_panel_kernel ------------------------------------------------------------------------------------------------
def ae_l1(M=65536, K=304, widths=(256, 256, 256, 256, 64, 64), **kw):
    """AE-30's first layer: six problems on ONE input (its magnitude slot too), relu, pre-cut planes."""
    A, am = P(), P()
    return [fwd(M, K, n, A=A, amax_a=am, **kw) for n in widths]


PIPE_FWD_128 = "gemm_pipe_kernel<true, true, 128, 0, 2, false, true>"
PIPE_FWD_64 = "gemm_pipe_kernel<true, true, 64, 0, 2, false, true>"


def test_panel_takes_the_first_layer():
    sym, grid, dyn, f = one("fwd", ae_l1())  # 512 panels of 128 rows on 256 compute units
    assert (sym, grid, dyn, f["rows"], f["masks"]) == ("gemm_panel_kernel", 256, 0, 65536, 0)
    assert one("fwd", ae_l1(masks=True))[3]["masks"] == 1
    assert brief("fwd", ae_l1(M=8192)) == ("gemm_panel_kernel", 64)
    for K in (160, 240, 320):
        assert brief("fwd", ae_l1(K=K))[0] == "gemm_panel_kernel"


def test_panel_ragged_batch():
    """65 536 rows to the panel kernel, the last 64 to the tile kernel: one row tile x (4 x 4 + 2 x 1) 64-wide column tiles
    (10 wide tiles would not fill the resident slots: 64-wide), all magnitudes and planes there.  (The call reports the
    panel kernel as its symbol: gemm.hip does not note a launch with row0 != 0.)"""
    launches, end = run("fwd", ae_l1(M=65536 + 64))
    assert end == "ok" and [s for s, _ in launches] == ["gemm_panel_kernel", PIPE_FWD_64]
    assert (launches[0][1]["grid"], launches[0][1]["rows"]) == (256, 65536)
    t = launches[1][1]
    assert (t["grid"], t["row0"], t["tiles_m"], t["total_ntiles"], t["count"]) == (18, 65536, 1, 18, 6)


def test_panel_refusals_name_the_tile_launch():
    # M = 8 191: 64 row tiles x 10 wide tiles = 640 < 1 024 -> 64-wide, 64 x 18 = 1 152 tiles on 3 x 256 slots
    assert brief("fwd", ae_l1(M=8191)) == (PIPE_FWD_64, 768)
    # at M = 65 536: 512 x 10 wide tiles, two resident workgroups per compute unit
    for K in (144, 336):
        assert brief("fwd", ae_l1(K=K)) == (PIPE_FWD_128, 512)
    d = ae_l1()
    d[5]["act"] = NONE  # (K = 304 is no reduction length of the weight-stationary kernel either)
    assert brief("fwd", d) == (PIPE_FWD_128, 512)
    sym, grid, _, f = one("fwd", ae_l1(widths=(256, 256, 256, 256, 64)))  # 17 halves
    assert (sym, grid, f["total_ntiles"]) == (PIPE_FWD_128, 512, 9)
    d = ae_l1()
    d[0]["relu_mask"] = P()
    assert brief("fwd", d) == (PIPE_FWD_128, 512)
    d = ae_l1()
    d[2].update(mul=P(), prod=P(), ldmul=256, ldprod=256)
    sym, grid, _, f = one("fwd", d)
    assert (sym, grid, f["k7"]) == (PIPE_FWD_128, 512, 1)
    d = ae_l1()
    d[3]["A"] = P()  # another input
    assert brief("fwd", d) == (PIPE_FWD_128, 512)
    assert brief("fwd", ae_l1(), panel=0) == (PIPE_FWD_128, 512)


# ---- gemm_ws_kernel ---------------------------------------------------------------------------------------------------
def l2(M=65536, K=256, N=128, n=4, **kw):
    return [fwd(M, K, N, **kw) for _ in range(n)]


def test_ws_forward():
    sym, grid, dyn, f = one("fwd", l2(masks=True))
    assert (sym, grid, dyn) == ("gemm_ws_kernel<4, 0, true, 4, false>", 256, 0)
    assert (f["n_prob"], f["wg_per_prob"], f["members"]) == (4, 64, "0,1,2,3")
    assert brief("fwd", l2()) == ("gemm_ws_kernel<4, 0, false, 4, false>", 256)
    assert brief("fwd", l2(K=240)) == ("gemm_ws_kernel<4, 0, false, 5, false>", 256)  # 240 = 3 x 80
    assert brief("fwd", l2(N=64, K=128, n=2)) == ("gemm_ws_kernel<2, 0, false, 4, false>", 256)  # the towers
    assert brief("fwd", l2(N=128, K=64, act=SIGMOID2, k7=True)) == ("gemm_ws_kernel<4, 0, false, 4, true>", 256)
    assert brief("fwd", l2(M=8269, w_kn=1)) == ("gemm_ws_kernel<4, 0, false, 4, false>", 256)  # (STAR's layers)
    assert brief("fwd", l2(n=3))[1] == 255  # 85 workgroups per problem


def test_ws_forward_refusals_name_the_tile_launch():
    assert brief("fwd", l2(K=304)) == (PIPE_FWD_128, 512)  # 512 x 4 wide tiles
    assert brief("fwd", l2(N=256, n=2)) == (PIPE_FWD_128, 512)  # 256 KiB of weight
    assert brief("fwd", l2(N=512, K=512, n=1)) == (PIPE_FWD_128, 512)
    # M = 8 191: 64 x 4 wide tiles < 1 024 -> 64-wide, 64 x 8 = 512 tiles
    assert brief("fwd", l2(M=8191)) == (PIPE_FWD_64, 512)
    assert brief("fwd", l2(), ws=0) == (PIPE_FWD_128, 512)
    assert brief("fwd", l2(), cus=3) == (PIPE_FWD_128, 6)  # n > compute units; two slots on each of three
    # K7 at N = 256: no instantiation -> the tile kernel's K7 form, one 512 x 2 launch
    sym, grid, _, f = one("fwd", l2(N=256, K=64, n=1, act=SIGMOID2, k7=True))
    assert (sym, grid, f["k7"]) == (PIPE_FWD_128, 512, 1)


def test_ws_classes_launch_in_the_order_of_their_first_members():
    d = [fwd(65536, 256, n) for n in (128, 64, 128, 64)]
    launches, end = run("fwd", d)
    assert end == "ok"
    assert [(s, f["members"], f["n_prob"], f["wg_per_prob"], f["grid"]) for s, f in launches] == [
        ("gemm_ws_kernel<4, 0, false, 4, false>", "0,2", 2, 128, 256),
        ("gemm_ws_kernel<2, 0, false, 4, false>", "1,3", 2, 128, 256)]
    d[2]["relu_mask"] = P()  # sign masks are a class of their own
    assert [f["members"] for _, f in run("fwd", d)[0]] == ["0", "1,3", "2"]


def test_ws_dgrad():
    d = [dgrad(65536, 256, [128]) for _ in range(4)]  # the input gradients of the second layers
    assert brief("dgrad", d) == ("gemm_ws_kernel<8, 1, false, 4, false>", 256)
    assert brief("dgrad", [dgrad(65536, 256, [128], masks=True) for _ in range(4)]) == \
        ("gemm_ws_kernel<8, 1, true, 4, false>", 256)
    assert brief("dgrad", [dgrad(65536, 128, [64]) for _ in range(2)]) == ("gemm_ws_kernel<4, 1, false, 4, false>", 256)
    assert brief("dgrad", [dgrad(65536, 64, [240])]) == ("gemm_ws_kernel<2, 1, false, 5, false>", 256)
    # two problems writing one dA need the call's order: the tile kernel (2 wide tiles x 512 rows = 1 024 -> 128-wide)
    d = [dgrad(65536, 128, [256]) for _ in range(2)]
    assert brief("dgrad", d)[0] == "gemm_ws_kernel<4, 1, false, 4, false>"
    d[1]["dA"] = d[0]["dA"]
    assert brief("dgrad", d) == ("gemm_pipe_kernel<true, false, 128, 1, 2, false, true>", 512)
    assert brief("dgrad", [dgrad(65536, 256, [128]) for _ in range(4)], cus=3)[0].startswith("gemm_pipe_kernel")


# ---- gemm_os_kernel ---------------------------------------------------------------------------------------------------
L1_NS = [256, 256, 256, 256, 64, 64]
PIPE_DGRAD_64 = "gemm_pipe_kernel<true, false, 64, 1, 2, false, true>"


def test_os_takes_the_input_gradient_of_the_first_layers():
    assert one("dgrad", [dgrad(16384, 240, L1_NS)])[:3] == ("gemm_os_kernel", 64, 0)  # 64 panels of 256 rows
    assert brief("dgrad", [dgrad(65536, 240, L1_NS)]) == ("gemm_os_kernel", 256)
    assert brief("dgrad", [dgrad(16384, 256, [128, 128])]) == ("gemm_os_kernel", 64)
    assert brief("dgrad", [dgrad(16384, 192, L1_NS)]) == ("gemm_os_kernel", 64)


def test_os_refusals_name_the_tile_launch():
    """All at 128 row tiles x 2 wide tiles < 1 024: 64-wide tiles, two resident workgroups per compute unit (dgrad)."""
    assert brief("dgrad", [dgrad(16383, 240, L1_NS)]) == (PIPE_DGRAD_64, 512)  # 128 x 4 tiles
    assert brief("dgrad", [dgrad(16384, 188, L1_NS)]) == (PIPE_DGRAD_64, 384)  # 128 x 3
    assert brief("dgrad", [dgrad(16384, 260, L1_NS)]) == (PIPE_DGRAD_64, 512)  # 128 x 5 on 512 slots
    assert brief("dgrad", [dgrad(16384, 240, [256])]) == (PIPE_DGRAD_64, 512)  # (240 is no width of the ws kernel)
    assert brief("dgrad", [dgrad(16384, 240, L1_NS, kexp=[P() for _ in L1_NS])]) == \
        ("gemm_pipe_kernel<true, false, 64, 1, 2, false, false>", 512)  # (nor does the tile kernel read the planes then)
    assert brief("dgrad", [dgrad(16384, 240, L1_NS, w_kn=1)]) == ("gemm_pipe_kernel<true, true, 64, 1, 2, false, true>", 512)
    assert brief("dgrad", [dgrad(16384, 240, L1_NS)], os=0) == (PIPE_DGRAD_64, 512)
    # N_s % 16 != 0: not even the LDS-DMA kernel
    assert brief("dgrad", [dgrad(16384, 240, [256, 256, 256, 256, 64, 72])]) == ("gemm_kernel<true, false, 64, 1>", 512)
    d = dgrad(16384, 240, L1_NS)
    d["src"][3].update(w_kn=1)
    assert run("dgrad", [d]) == ([], ("refused", -1, "mml_gemm_grouped_dgrad: mixed weight layouts inside problem 0"))


# ---- gemm_nt_kernel ---------------------------------------------------------------------------------------------------
def ae_l1_wgrad(M=65536, **kw):
    return [wgrad(M, n, 304, **kw) for n in (256, 256, 256, 256, 64, 64)]


AE_L1_SLAB_BYTES = 4 * (4 * (256 * 304 + 256) + 2 * (64 * 304 + 64))  # one slab of the nt kernel: dW and dbias partials
PIPE_WGRAD_64 = "gemm_pipe_kernel<false, false, 64, 2, 2, false, false>"
PIPE_WGRAD_128 = "gemm_pipe_kernel<false, false, 128, 2, 2, false, false>"


def test_nt_slabs_and_grid():
    assert AE_L1_SLAB_BYTES == 1405440
    # 4 x (2 x 3) + 2 x (1 x 3) = 30 tiles; 2 x 256 / 30 = 17 slabs
    sym, grid, dyn, f = one("wgrad", ae_l1_wgrad())
    assert (sym, grid, dyn, f["slabs"], f["tiles"], f["partials"], f["reduce"]) == ("gemm_nt_kernel", 510, 0, 17, 30, 1, 1)
    f = one("wgrad", ae_l1_wgrad(), phase=1)[3]
    assert (f["slabs"], f["partials"], f["reduce"]) == (17, 1, 0)
    f = one("wgrad", ae_l1_wgrad(), phase=2)[3]
    assert (f["slabs"], f["partials"], f["reduce"]) == (17, 0, 1)
    assert one("wgrad", ae_l1_wgrad(), ws_bytes=5 * AE_L1_SLAB_BYTES + 100)[3]["slabs"] == 5  # what the workspace holds
    # not even one slab: the tile kernel's call, which then misses its own workspace
    assert run("wgrad", ae_l1_wgrad(), ws_bytes=AE_L1_SLAB_BYTES - 4) == (
        [], ("refused", -1, "mml_gemm_grouped_wgrad: workspace 1405436 < 23892480 bytes"))
    # one tile: 512 slabs by the compute units; 16 384 rows are 512 steps -> 64 slabs of 8 steps; and never more than 64
    assert brief("wgrad", [wgrad(16384, 64, 64)]) == ("gemm_nt_kernel", 64)
    assert brief("wgrad", [wgrad(65536, 64, 64)]) == ("gemm_nt_kernel", 64)
    sym, grid, dyn, f = one("wgrad", ae_l1_wgrad(), per_cu=1)  # 256 / 30 = 8 slabs, one workgroup per compute unit
    assert (sym, grid, dyn, f["slabs"]) == ("gemm_nt_kernel", 240, 20480, 8)
    assert one("wgrad", ae_l1_wgrad(), nt=3)[:3] == ("gemm_nt_kernel", 510, 0)  # (the lab variant reports the same symbol)
    assert brief("wgrad", ae_l1_wgrad(), nt=2) == ("gemm_nt_kernel", 510)  # 30 >= 16 tiles


def test_nt_refusals_name_the_tile_launch():
    """One 128 x 128 problem on the tile kernel at M = 65 536: 256 chunk rows x 1 wide tile < 1 024 -> 64-wide, 2 tiles;
    768 / 2 = 384 splits, at most one per 256 batch rows -> S = 256 chunks of 256 rows."""
    sym, grid, dyn, f = one("wgrad", [wgrad(65536, 128, 128)], nt=2)  # 1 tile < 16
    assert (sym, grid, dyn) == (PIPE_WGRAD_64, 512, 0)
    assert (f["S"], f["chunk"], f["slab_floats"], f["ws_off"]) == (256, 256, 256 * (128 * 128 + 128), 0)
    assert brief("wgrad", [wgrad(65536, 128, 128)], nt=0) == (PIPE_WGRAD_64, 512)
    # M % 32 != 0: 257 chunks of 256 rows
    sym, grid, _, f = one("wgrad", [wgrad(65536 + 16, 128, 128)])
    assert (sym, grid, f["S"], f["chunk"], f["slab_floats"]) == (PIPE_WGRAD_64, 514, 257, 256, 257 * 16512)
    sym, grid, _, f = one("wgrad", [wgrad(65536, 72, 128)])  # N % 32 != 0
    assert (sym, grid, f["slab_floats"]) == (PIPE_WGRAD_64, 512, 256 * (72 * 128 + 72))
    # a missing magnitude: three bf16 planes
    assert brief("wgrad", [wgrad(65536, 128, 128, amax_a=0)]) == ("gemm_pipe_kernel<false, false, 64, 2, 3, false, false>", 512)
    assert brief("wgrad", [wgrad(16352, 128, 128)])[0] == PIPE_WGRAD_64  # M < 16 384
    assert brief("wgrad", [wgrad(65536, 128, 128, w_kn=1)])[0] == "gemm_pipe_kernel<false, false, 64, 2, 2, true, false>"
    # n = 49: three runs of 16 (16 wide tiles, 512 / 16 = 32 chunks of 2 048 rows) and one of 1, each with its own piece
    launches, end = run("wgrad", [wgrad(65536, 128, 128) for _ in range(49)])
    assert end == "ok"
    assert [(s, f["grid"], f["first"], f["count"], f["S"], f["chunk"], f["ws_off"]) for s, f in launches] == [
        (PIPE_WGRAD_128, 512, 0, 16, 32, 2048, 0), (PIPE_WGRAD_128, 512, 16, 16, 32, 2048, 33816576),
        (PIPE_WGRAD_128, 512, 32, 16, 32, 2048, 67633152), (PIPE_WGRAD_64, 512, 48, 1, 256, 256, 101449728)]
    assert brief("wgrad", [wgrad(65536, 128, 128) for _ in range(48)])[0] == "gemm_nt_kernel"


# ---- the tile kernels -------------------------------------------------------------------------------------------------
def wide(M=65536, **kw):
    """One 512 -> 256 layer: too long for the panel kernel, too large for the weight-stationary one."""
    return [fwd(M, 512, 256, **kw)]


def test_register_staged_kernel_where_the_lds_dma_cannot_go():
    assert one("fwd", [fwd(1000, 100, 64, act=NONE)])[:3] == ("gemm_kernel<true, true, 64, 0>", 8, 0)  # K % 16 != 0
    d = fwd(1000, 128, 64)
    d["A"] += 4
    assert brief("fwd", [d]) == ("gemm_kernel<true, true, 64, 0>", 8)
    assert brief("fwd", [fwd(1000, 128, 64)]) == (PIPE_FWD_64, 8)
    assert brief("fwd", [fwd(1000, 128, 64)], glds=0) == ("gemm_kernel<true, true, 64, 0>", 8)
    assert brief("fwd", [fwd(1000, 128, 66, w_kn=1)]) == ("gemm_kernel<true, false, 64, 0>", 16)  # N % 4 != 0, [K, N]
    assert brief("wgrad", [wgrad(1000, 64, 128)])[0] == "gemm_kernel<false, false, 64, 2>"  # the batch: 1 000 % 16 != 0
    assert brief("dgrad", [dgrad(1000, 64, [100])])[0] == "gemm_kernel<true, false, 64, 1>"


def test_tile_width():
    # more than a third of a wide tile's columns would be padding (64 of 128), however many rows
    assert brief("fwd", [fwd(4 * 65536, 128, 64)], ws=0) == (PIPE_FWD_64, 768)
    assert brief("fwd", [fwd(4 * 65536, 128, 128)], ws=0) == (PIPE_FWD_128, 512)
    assert brief("fwd", [fwd(4 * 65536, 128, 192)], ws=0) == (PIPE_FWD_128, 512)  # 192 of 256: a quarter
    # 512 row tiles x 2 wide tiles fill the 512 slots twice, 511 x 2 do not
    assert brief("fwd", wide()) == (PIPE_FWD_128, 512)
    assert brief("fwd", wide(M=65536 - 128)) == (PIPE_FWD_64, 768)
    assert brief("fwd", [fwd(1000, 128, 64)], bn=128) == (PIPE_FWD_128, 8)
    assert brief("fwd", wide(), bn=64) == (PIPE_FWD_64, 768)
    assert brief("fwd", wide(), bn=32) == (PIPE_FWD_128, 512)


def test_arithmetic():
    sym = "gemm_pipe_kernel<true, true, 128, 0, %d, false, %s>"
    assert brief("fwd", wide(), mode=0)[0] == sym % (0, "false")
    assert brief("fwd", wide(), mode=1)[0] == sym % (1, "false")
    assert brief("fwd", wide(), mode=3)[0] == sym % (3, "false")
    assert brief("fwd", wide(), mode=2)[0] == sym % (2, "true")
    assert brief("fwd", wide(), mode=4)[0] == sym % (2, "true")
    assert brief("fwd", wide(amax_w=0))[0] == sym % (3, "false")
    assert brief("fwd", wide(amax_a=0))[0] == sym % (3, "false")
    d = [dgrad(65536, 512, [256, 256])]
    d[0]["src"][1]["amax_dc"] = 0
    assert brief("dgrad", d)[0] == "gemm_pipe_kernel<true, false, 128, 1, 3, false, false>"


def test_precut_planes():
    sym = "gemm_pipe_kernel<true, true, 128, 0, 2, false, %s>"
    assert brief("fwd", wide())[0] == sym % "true"
    assert brief("fwd", wide(), planes=0)[0] == sym % "false"
    assert brief("fwd", wide(w_planes=0))[0] == sym % "false"
    assert brief("fwd", wide(w_kexp=0))[0] == sym % "false"
    d = wide()
    d[0]["w_planes"] += 8
    assert brief("fwd", d)[0] == sym % "false"
    assert brief("fwd", wide() + wide(w_planes=0))[0] == sym % "false"  # every problem of the launch or none


def test_grid_is_capped_at_the_resident_slots():
    assert brief("fwd", wide()) == (PIPE_FWD_128, 512)
    assert brief("fwd", wide(), cus=304) == (PIPE_FWD_128, 608)
    assert brief("fwd", [fwd(131072, 128, 64)], ws=0) == (PIPE_FWD_64, 768)
    assert brief("fwd", [fwd(131072, 128, 64, act=SIGMOID2, k7=True)], ws=0) == (PIPE_FWD_64, 512)
    assert brief("dgrad", [dgrad(131072, 64, [128])], ws=0) == (PIPE_DGRAD_64, 512)
    assert brief("fwd", [fwd(300, 128, 64)]) == (PIPE_FWD_64, 3)
    assert run("fwd", [fwd(0, 128, 64)]) == ([], "ok")  # nothing to launch
    assert run("fwd", []) == ([], "ok")


def gate(M, K, N, **kw):
    """A gate-mode input gradient (PepNet): d_h, d_g instead of dA."""
    return dgrad(M, K, [N], dA=0, gate_h=P(), gate_g=P(), d_h=P(), d_g=P(), ld_h=K, ld_g=K, ld_dh=K, ld_dg=K, act_g=SIGMOID2,
                 **kw)


def test_k7():
    assert brief("fwd", [fwd(2048, 96, 128, act=SIGMOID2, k7=True)]) == (PIPE_FWD_64, 32)  # (test_pep_gate_gpu's sizes)
    sym, grid, _, f = one("dgrad", [gate(131072, 256, 64)])  # gate mode: narrow tiles whatever pick_tiles says
    assert (sym, grid, f["k7"], f["bn"]) == (PIPE_DGRAD_64, 512, 1, 64)
    assert brief("dgrad", [gate(65536, 128, 64)])[0] == "gemm_ws_kernel<4, 1, false, 4, true>"
    assert run("fwd", [fwd(2048, 96, 128, act=SIGMOID2, k7=True)], mode=0) == (
        [], ("refused", -3, "mml_gemm_grouped_fwd: the K7 products run on the plane-emulated GEMM forms only"))
    assert run("fwd", [fwd(2048, 96, 128, act=SIGMOID2, k7=True, w_kn=1)]) == (
        [], ("refused", -3, "mml_gemm_grouped_fwd: the K7 products need nn.Linear weights ([N, K])"))
    assert run("dgrad", [gate(2048, 128, 64, w_kn=1)]) == (
        [], ("refused", -3, "mml_gemm_grouped_dgrad: the K7 products need nn.Linear weights ([N, K])"))
    assert run("fwd", [fwd(2048, 100, 128, act=SIGMOID2, k7=True)]) == (
        [], ("refused", -3, "mml_gemm_grouped_fwd: mul / prod need the LDS-DMA kernel (K % 16 == 0, 16-byte aligned "
                             "operands)"))
    assert run("dgrad", [gate(2048, 128, 72)]) == (
        [], ("refused", -3, "mml_gemm_grouped_dgrad: gate mode needs the LDS-DMA kernel (N_s % 16 == 0, 16-byte aligned "
                             "operands)"))


def test_wgrad_plan_and_workspace():
    """AE-30's first layer on the tile kernel: 6 x 3 wide tiles of columns (304 -> 384), 2 row tiles x 256 chunk rows ->
    128-wide; 30 tiles, 512 / 30 = 17 splits of ceil(65 536 / 17 = 3 856 / 32) x 32 = 3 872 rows."""
    floats = 17 * (4 * 256 * 304 + 2 * 64 * 304 + 4 * 256 + 2 * 64)
    assert floats == 5973120
    sym, grid, dyn, f = one("wgrad", ae_l1_wgrad(), nt=0)
    assert (sym, grid, dyn) == (PIPE_WGRAD_128, 510, 0)
    assert (f["S"], f["chunk"], f["slab_floats"], f["total_ntiles"], f["partials"], f["reduce"]) == (17, 3872, floats, 30, 1, 1)
    assert run("wsbytes", ae_l1_wgrad())[1] == ("bytes", floats * 4 + 256)
    assert one("wgrad", ae_l1_wgrad(), nt=0, pad=17408)[2] == 17408
    f = one("wgrad", ae_l1_wgrad(), nt=0, phase=2)[3]
    assert (f["S"], f["partials"], f["reduce"]) == (17, 0, 1)
    assert run("wgrad", ae_l1_wgrad(), nt=0, ws_bytes=floats * 4 - 4) == (
        [], ("refused", -1, "mml_gemm_grouped_wgrad: workspace %d < %d bytes" % (floats * 4 - 4, floats * 4)))
    # one small group: 64 x 128 at M = 4 096 -> 2 narrow tiles, 16 chunks of 256 rows
    sym, grid, _, f = one("wgrad", [wgrad(4096, 64, 128)])
    assert (sym, grid, f["S"], f["chunk"], f["slab_floats"]) == (PIPE_WGRAD_64, 32, 16, 256, 16 * (64 * 128 + 64))
    assert run("wsbytes", [wgrad(4096, 64, 128)])[1] == ("bytes", 16 * (64 * 128 + 64) * 4 + 256)
    # two groups (another batch size): one piece of the workspace each, rounded up to 256 bytes
    two = [wgrad(4096, 64, 128), wgrad(2048, 64, 100, dbias=0)]
    launches, end = run("wgrad", two)
    assert end == "ok" and [(f["first"], f["S"], f["ws_off"]) for _, f in launches] == [(0, 16, 0), (1, 8, 528384)]
    assert run("wsbytes", two)[1] == ("bytes", 528384 + 8 * 64 * 100 * 4 + 256)


def test_runs_of_a_forward_call():
    d = [fwd(1000, 128, 64) for _ in range(17)] + [fwd(1000, 128, 64, w_kn=1), fwd(2000, 128, 64, w_kn=1)]
    launches, end = run("fwd", d)
    assert end == "ok" and [(f["first"], f["count"]) for _, f in launches] == [(0, 16), (16, 1), (17, 1), (18, 1)]
    d[17]["W"] = 0  # a refusal behind launches that already went out
    launches, end = run("fwd", d)
    assert len(launches) == 2 and end == ("refused", -1, "mml_gemm_grouped_fwd: null pointer in problem 17")
    # dgrad: at most 24 sources per launch
    d = [dgrad(1000, 64, [128] * 8) for _ in range(4)]
    assert [(f["first"], f["count"]) for _, f in run("dgrad", d)[0]] == [(0, 3), (3, 1)]
    d[1]["n_src"] = 9
    assert run("dgrad", d)[1] == ("refused", -1, "mml_gemm_grouped_dgrad: problem 1 malformed")


# ---- the modes --------------------------------------------------------------------------------------------------------
def test_only_the_auto_modes_reach_the_plane_kernels():
    calls = [("fwd", ae_l1()), ("fwd", l2()), ("dgrad", [dgrad(65536, 256, [128]) for _ in range(4)]),
             ("dgrad", [dgrad(16384, 240, L1_NS)]), ("wgrad", ae_l1_wgrad())]
    for kind, d in calls:
        for mode in (2, 4):
            assert brief(kind, d, mode=mode)[0].split("<")[0] in ("gemm_panel_kernel", "gemm_ws_kernel", "gemm_os_kernel",
                                                                  "gemm_nt_kernel"), (kind, mode)
        for mode in (0, 1, 3):
            sym = brief(kind, d, mode=mode)[0]
            assert sym.startswith("gemm_pipe_kernel<") and ", %d, false, false>" % mode in sym, (kind, mode, sym)


# ---- the shapes the device tests launch and read the symbol of ------------------------------------------------------------
def test_shapes_of_the_device_tests():
    # test_gemm_panel_gpu.py
    assert brief("fwd", ae_l1(M=8192, K=240, masks=True)) == ("gemm_panel_kernel", 64)
    assert brief("fwd", ae_l1(M=8192, K=240, widths=(256, 64, 64))) == ("gemm_panel_kernel", 64)
    for M, K, N in ((8192, 336, 128), (8192, 144, 128), (4096, 240, 128), (8192 + 77 - 128, 240, 128), (8192, 240, 192)):
        assert brief("fwd", [fwd(M, K, N)], ws=0)[0].startswith("gemm_pipe_kernel<true, true, 64, 0, 2,"), (M, K, N)
    for act in (NONE, 2):
        assert brief("fwd", [fwd(8192, 240, 128, act=act)], ws=0)[0] == PIPE_FWD_64
    # test_gemm_ws_gpu.py
    assert brief("fwd", l2(K=128, N=64, n=2, masks=True)) == ("gemm_ws_kernel<2, 0, true, 4, false>", 256)
    for M, K, N in ((8192, 512, 128), (8192, 208, 128), (4096, 256, 128), (8192, 256, 256), (8192, 128, 192)):
        assert not brief("fwd", [fwd(M, K, N, act=NONE)])[0].startswith("gemm_ws_kernel"), (M, K, N)
    assert brief("fwd", l2(K=64, N=64, act=SIGMOID2, k7=True)) == ("gemm_ws_kernel<2, 0, false, 4, true>", 256)
    assert brief("fwd", l2(M=8192 + 77, K=128, N=128, n=3, act=SIGMOID2, k7=True)) == ("gemm_ws_kernel<4, 0, false, 4, true>", 255)
    assert brief("dgrad", [gate(65536, 64, 128) for _ in range(4)]) == ("gemm_ws_kernel<2, 1, false, 4, true>", 256)
    assert brief("dgrad", [gate(8192 + 77, 128, 128, act_h=RELU) for _ in range(3)]) == \
        ("gemm_ws_kernel<4, 1, false, 4, true>", 255)
    # test_gemm_os_gpu.py
    assert brief("dgrad", [dgrad(65536, 240, L1_NS, accumulate=1)]) == ("gemm_os_kernel", 256)
    assert brief("dgrad", [dgrad(16384, 256, [128])]) == ("gemm_ws_kernel<8, 1, false, 4, false>", 256)
    for M, K, Ns in ((8192, 240, [256, 64]), (16384, 240, [64, 64]), (16384, 288, [256, 256]), (16384, 128, [256, 256])):
        assert brief("dgrad", [dgrad(M, K, Ns)])[0].startswith("gemm_pipe_kernel<true, false, 64, 1, 2, false, true>"), (M, K, Ns)
    # test_gemm_nt_gpu.py
    assert brief("wgrad", [wgrad(65536, n, 240) for n in (256, 256, 256, 256, 64, 64)]) == ("gemm_nt_kernel", 500)  # 20 tiles x 25
    assert brief("wgrad", [wgrad(65536, 128, 256) for _ in range(4)]) == ("gemm_nt_kernel", 512)  # 8 tiles x 64 slabs
    assert brief("wgrad", [wgrad(16384 + 32 * 5, 96, 100), wgrad(16384 + 32 * 5, 32, 4)]) == ("gemm_nt_kernel", 128)
    # test_gemm_pipe_gpu.py, test_pep_gate_gpu.py, test_star_linear_gpu.py: small batches on the tile kernels
    assert brief("fwd", [fwd(300, 64, 96, w_kn=1)])[0] == "gemm_pipe_kernel<true, false, 64, 0, 2, false, true>"
    assert brief("fwd", [fwd(300, 50, 96)])[0] == "gemm_kernel<true, true, 64, 0>"


def wg(M, shapes, amax=True, w_kn=0, **knobs):
    """The reported symbol of a weight-gradient call over (N, K) shapes, in a workspace of the size the library asks for
    (what ops.gemm_wgrad does)."""
    kw = {} if amax else dict(amax_dc=0, amax_a=0)
    d = [wgrad(M, N, K, w_kn=w_kn, **kw) for N, K in shapes]
    launches, end = run("wgrad", d, ws_bytes=run("wsbytes", d, **knobs)[1][1], **knobs)
    assert end == "ok"
    return launches[-1][0]


def test_shapes_of_test_gemm_nt_gpu():
    AE = [(256, 240)] * 4 + [(64, 240)] * 2
    PEP = [(64, 72), (96, 80), (32, 64), (128, 128)] * 12
    for M, shapes in ((65536, AE), (65536, [(128, 256)] * 4), (65536, [(64, 128)] * 2), (16384, [(256, 304), (64, 304)]),
                      (16384 + 32 * 5, [(96, 100), (32, 4)]), (32768, [(512, 512), (128, 512)]), (16384, PEP),
                      (32768, [(32, 8)] * 41), (16384, [(128, 256), (64, 256)]), (32768, [(256, 240), (64, 240)])):
        assert wg(M, shapes) == "gemm_nt_kernel", (M, shapes)
    for M, shapes in ((65536, AE), (16384 + 32 * 5, [(96, 100), (32, 4)]), (16384, PEP)):
        assert wg(M, shapes, nt=3) == "gemm_nt_kernel", (M, shapes)
    # nt = 0: two 128-wide tiles of columns x 2 row tiles x 128 chunk rows = 1 024 -> 128-wide
    assert wg(32768, [(256, 240), (64, 240)], nt=0) == PIPE_WGRAD_128
    # what it leaves to the tile kernel (all of them few tiles: 64-wide)
    for M, shapes in ((8192, [(128, 256)]), (16384, [(32, 16)] * 49), (16384 + 16, [(128, 256)]), (16384, [(100, 48)])):
        assert wg(M, shapes) == PIPE_WGRAD_64, (M, shapes)
    assert wg(16384, [(128, 256)], amax=False) == "gemm_pipe_kernel<false, false, 64, 2, 3, false, false>"


def test_shapes_of_test_gemm_ws_gpu():
    # input gradients: (M, reduction, width, problems, [K, N] layout, sign masks)
    for M, Nred, K, n, kn, relu, sym in (
            (65536, 128, 256, 4, 0, True, "gemm_ws_kernel<8, 1, true, 4, false>"),
            (65536, 64, 128, 2, 0, False, "gemm_ws_kernel<4, 1, false, 4, false>"),
            (8192 + 77, 128, 256, 3, 0, True, "gemm_ws_kernel<8, 1, true, 4, false>"),
            (16384 + 5, 192, 128, 5, 1, True, "gemm_ws_kernel<4, 1, true, 4, false>"),
            (8192, 64, 256, 1, 0, False, "gemm_ws_kernel<8, 1, false, 4, false>"),
            (8192 + 96, 128, 64, 4, 0, True, "gemm_ws_kernel<2, 1, true, 4, false>"),
            (8192, 80, 128, 2, 0, True, "gemm_ws_kernel<4, 1, true, 5, false>")):
        d = [dgrad(M, K, [Nred], w_kn=kn, masks=relu) for _ in range(n)]
        assert brief("dgrad", d)[0] == sym, (M, Nred, K)
        assert brief("dgrad", d, ws=0)[0].startswith("gemm_pipe_kernel<true, %s, " % ("true" if kn else "false")), (M, Nred, K)
    assert brief("dgrad", [dgrad(65536, 256, [128]) for _ in range(4)])[0].startswith("gemm_ws_kernel")
    # two sources; a derivative from the stored outputs; a width that is not instantiated
    assert brief("dgrad", [dgrad(8192, 256, [128, 128], masks=True)])[0] == PIPE_DGRAD_64
    assert brief("dgrad", [dgrad(8192, 256, [128], act=RELU, Y=P(), ldy=256)])[0] == PIPE_DGRAD_64
    assert brief("dgrad", [dgrad(8192, 192, [64])])[0] == PIPE_DGRAD_64
    # K7 forward and gate-mode input gradients, with the kernel on and off
    for M, K, N, n, sym in ((65536, 64, 64, 4, "gemm_ws_kernel<2, 0, false, 4, true>"),
                            (8192 + 77, 128, 128, 3, "gemm_ws_kernel<4, 0, false, 4, true>"),
                            (16384, 80, 64, 2, "gemm_ws_kernel<2, 0, false, 5, true>")):
        d = l2(M=M, K=K, N=N, n=n, act=SIGMOID2, k7=True)
        assert brief("fwd", d)[0] == sym
        assert brief("fwd", d, ws=0)[0] == PIPE_FWD_64
    for M, Nred, K, n, sym in ((65536, 128, 64, 4, "gemm_ws_kernel<2, 1, false, 4, true>"),
                               (8192 + 77, 128, 128, 3, "gemm_ws_kernel<4, 1, false, 4, true>"),
                               (8192, 128, 64, 1, "gemm_ws_kernel<2, 1, false, 4, true>"),
                               (16384, 80, 128, 2, "gemm_ws_kernel<4, 1, false, 5, true>")):
        d = [gate(M, K, Nred) for _ in range(n)]
        assert brief("dgrad", d)[0] == sym
        sym_t, _, _, f = one("dgrad", d, ws=0)
        assert (sym_t, f["k7"]) == (PIPE_DGRAD_64, 1)


def test_shapes_of_test_gemm_pipe_gpu():
    """Launches without pre-cut planes; magnitudes only where the test passes them (mode 2)."""
    bare = dict(w_planes=0, w_kexp=0)
    for mode in (0, 3, 2):
        am = {} if mode == 2 else dict(amax_a=0, amax_w=0)
        emu = ", %d, false, false>" % mode
        for M, K, Ns in ((128, 16, [64]), (300, 32, [128, 4]), (4096 + 37, 48, [100]), (1000, 240, [256, 256, 64]),
                         (260, 64, [130]), (70000, 128, [128, 128])):
            A = P()
            sym = brief("fwd", [fwd(M, K, N, A=A, act=i % 4, **bare, **am) for i, N in enumerate(Ns)], mode=mode)[0]
            assert sym.startswith("gemm_pipe_kernel<true, true, ") and sym.endswith(", 0" + emu), (mode, M, K, Ns, sym)
        for M, K, Ns, kn in ((128, 64, [16], 0), (515, 256, [128], 0), (515, 240, [256, 256, 64, 64], 0), (515, 128, [64, 32], 0),
                             (300, 100, [48], 0), (300, 128, [48, 16], 1), (70000, 128, [128], 0)):
            d = dgrad(M, K, Ns, w_kn=kn, act=RELU, Y=P(), ldy=K)
            for s in d["src"]:
                s.update(w_planes=0, w_kexp=0, **({} if mode == 2 else dict(amax_dc=0, amax_w=0)))
            sym = brief("dgrad", [d], mode=mode)[0]
            assert sym.startswith("gemm_pipe_kernel<true, %s, " % ("true" if kn else "false")) and sym.endswith(", 1" + emu), sym
        for M, shapes, kn in ((4096, [(64, 16)], 0), (4096 + 16, [(256, 240), (64, 240)], 0), (8192, [(128, 256), (4, 64)], 0),
                              (8192, [(100, 48)], 0), (8192, [(64, 128), (64, 128)], 1), (70000, [(256, 240)], 0)):
            sym = wg(M, shapes, amax=mode == 2, w_kn=kn, mode=mode)
            assert sym.startswith("gemm_pipe_kernel<false, false, ") and \
                sym.endswith(", 2, %d, %s, false>" % (mode, "true" if kn else "false")), (mode, M, shapes, sym)
    assert brief("fwd", [fwd(200, 24, 96, **bare)])[0] == "gemm_kernel<true, true, 64, 0>"  # K % 16 != 0
    assert ", 2, " in brief("fwd", [fwd(1000, 240, 256, **bare)])[0]
    assert ", 3, " in brief("fwd", [fwd(1000, 240, 256, amax_a=0, amax_w=0, **bare)])[0]
    assert ", 2, " in brief("fwd", [fwd(1024, 240, 256, **bare)])[0]
    # pre-cut planes (the weight-stationary kernel switched off): honoured where the switch is on
    for planes in (1, 0):
        tail = ", 2, false, %s>" % ("true" if planes else "false")
        for M, K, Ns in ((1000, 240, [256, 256, 64]), (70000, 128, [128, 128]), (300, 32, [128, 4]), (4096 + 37, 48, [100])):
            A = P()
            assert brief("fwd", [fwd(M, K, N, A=A, act=NONE) for N in Ns], ws=0, planes=planes)[0].endswith(tail), (M, K, Ns)
        for M, K, Ns in ((1000, 240, [256, 256, 64, 64]), (70000, 256, [128]), (300, 64, [48, 16])):
            assert brief("dgrad", [dgrad(M, K, Ns)], ws=0, planes=planes)[0].endswith(tail), (M, K, Ns)
