"""model_name "pcg" (PCGrad, reference model/optimizer.py:10-138), the parts that need no GPU: the host-side order drawing
against Python's random.shuffle, what compile() accepts and refuses, the descriptor layout against the C compiler, and a
float64 numpy restatement of the wrapper's projection and merge, written here, which checks the fixtures of
tests/golden/make_golden_pcgrad.py without the code under test."""
import ctypes
import json
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, load_golden

RTOL = 1e-4
PCG_CASES = ["pcg_mmoe_mtl", "pcg_mmoe_t3"]


def cpu_build(g, objectives=None, model_name=None, **model_kw):
    import mmlrec_amd  # noqa: F401
    import torch
    from mmlrec_amd.model import MMOE, DenseFeat, SparseFeat
    cfg = json.loads(str(g["cfg"]))
    cfg["model_config"].update(model_kw)
    if model_name is not None:
        cfg["model_config"]["model_name"] = model_name
    if objectives is not None:
        cfg["optim_config"]["pcgrad_objectives"] = objectives
    emb = cfg["model_config"]["emb"]
    cols = [SparseFeat(str(n), int(v), embedding_dim=emb) for n, v in zip(g["sparse_names"], g["vocab"])]
    cols += [DenseFeat(str(n), 1) for n in g["dense_names"]]
    torch.manual_seed(0)
    return MMOE(cols, device="cpu", config=cfg), cfg


def project64(g, has, orders):
    """The wrapper's `_project_conflicting` in float64 numpy: g [T, n] per-objective flattened gradients, has [T, n] 0 / 1,
    orders[i] = the order in which g_i meets the g_j.  Every dot product is taken on the partly projected vector, as the
    reference does.  Returns (merged [n], dots [T, T] by position in the order, fired [T, T] by (i, j), norms of pc_i at
    each comparison [T, T])."""
    T = g.shape[0]
    pc = g.astype(np.float64).copy()
    g = g.astype(np.float64)
    dots, fired, norms = np.zeros((T, T)), np.zeros((T, T), dtype=np.int32), np.zeros((T, T))
    for i in range(T):
        for q, j in enumerate(orders[i]):
            d = float(pc[i] @ g[j])
            dots[i, q], norms[i, q] = d, float(np.linalg.norm(pc[i]))
            if d < 0:
                pc[i] = pc[i] - d * g[j] / float(g[j] @ g[j])
                fired[i, j] = 1
    shared = has.prod(0).astype(bool)
    return np.where(shared, pc.mean(0), pc.sum(0)), dots, fired, norms


def weights64(G, orders):
    """The same loop on coefficients over the Gram matrix of the ORIGINAL gradients (what mml_pcgrad_weights runs):
    pc_i = sum_k c[i, k] g_k.  Returns (c [T, T], fired [T, T])."""
    T = G.shape[0]
    c, fired = np.eye(T), np.zeros((T, T), dtype=np.int32)
    for i in range(T):
        for j in orders[i]:
            d = 0.0
            for k in range(T):
                d = d + c[i, k] * G[k, j]
            if d < 0 and G[j, j] > 0:
                c[i, j] -= d / G[j, j]
                fired[i, j] = 1
    return c, fired


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def elem_rel(a, b, floor=1e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.abs(a - b) / (RTOL * np.abs(b) + floor * max(np.abs(b).max(), 1e-30))).max()


def param_names(g):
    return [k[5:] for k in g.files if k.startswith("grad/")]


@pytest.mark.parametrize("T", [2, 3, 4])
def test_host_orders_are_random_shuffle_on_one_list(T):
    """T calls to random.shuffle per step on ONE T-element list that starts in task order at every step: under the same
    seed the port's draws are the reference's, step after step."""
    from mmlrec_amd.trainer import draw_pcgrad_orders
    random.seed(1234 + T)
    got = [draw_pcgrad_orders(T) for _ in range(5)]
    random.seed(1234 + T)
    for step in range(5):
        lst = list(range(T))
        for i in range(T):
            random.shuffle(lst)
            assert got[step][i] == lst, (step, i)
    assert len({tuple(map(tuple, o)) for o in got}) > 1  # (the seeds above do not draw one order five times)


@pytest.mark.parametrize("name", PCG_CASES)
def test_fixture_orders_are_the_seeded_draws(name):
    from mmlrec_amd.trainer import draw_pcgrad_orders
    g = load_golden(name)
    T = g["orders"].shape[1]
    random.seed(int(g["seed"]))
    for s in range(3):
        assert draw_pcgrad_orders(T) == g["orders"][s].tolist(), s


@pytest.mark.parametrize("objectives", [None, "total", "per_task"])
def test_compile_accepts_pcg(objectives):
    g = load_golden("pcg_mmoe_mtl")
    model, cfg = cpu_build(g, objectives)
    assert cfg["model_config"]["model_name"] == "pcg"
    model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
    assert model._pcgrad_objectives() == (objectives or "total")
    assert list(model.state_dict()) == [k[6:] for k in g.files if k.startswith("state/")]  # MMoE's keys


@pytest.mark.parametrize("key", ["l2_reg_embedding", "l2_reg_dnn"])
def test_per_task_with_a_regulariser_is_refused(key):
    g = load_golden("pcg_mmoe_mtl")
    model, cfg = cpu_build(g, "per_task", **{key: 1e-4})
    with pytest.raises(ValueError, match="regulariser"):
        model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
    model, cfg = cpu_build(g, "total", **{key: 1e-4})  # (the MMoE step carries the regulariser as ever)
    model.compile("adam", cfg["optim_config"]["loss"], ["auc"])


def test_the_key_is_refused_on_other_models_and_values():
    g = load_golden("pcg_mmoe_mtl")
    model, cfg = cpu_build(g, "per_task", model_name="mmoe")
    with pytest.raises(ValueError, match="pcg"):
        model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
    model, cfg = cpu_build(g, "total", model_name="mmoe")
    model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
    model, cfg = cpu_build(g, "sum")
    with pytest.raises(ValueError, match="pcgrad_objectives"):
        model.compile("adam", cfg["optim_config"]["loss"], ["auc"])


def test_shard_model_refuses_per_task():
    from mmlrec_amd import parallel
    g = load_golden("pcg_mmoe_mtl")
    model, cfg = cpu_build(g, "per_task")
    with pytest.raises(NotImplementedError, match="one GPU"):
        parallel.shard_model(model, None, mode="replicated")


def test_descriptor_layout_matches_the_header():
    from mmlrec_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mmlrec.h"\nint main(){printf("%zu %zu %zu %d\\n", '
           'sizeof(mml_pcgrad_seg), offsetof(mml_pcgrad_seg, out), offsetof(mml_pcgrad_seg, row_marks), '
           'MML_PCGRAD_MAX_TASKS);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size, off_out, off_marks, maxt = map(int, subprocess.check_output([exe]).decode().split())
    S = _lib.PcgradSeg
    assert (ctypes.sizeof(S), S.out.offset, S.row_marks.offset, _lib.PCGRAD_MAX_TASKS) == (size, off_out, off_marks, maxt)


@pytest.mark.parametrize("name", PCG_CASES)
def test_float64_restatement_reproduces_the_fixture(name):
    """Dots, fired flags and the merged gradient of step 0 from the stored per-objective gradients; and the coefficient
    form over their Gram matrix -- the port's formulation -- gives the same flags and the same merged gradient."""
    g = load_golden(name)
    names = param_names(g)
    T = g["orders"].shape[1]
    gt = np.stack([np.concatenate([g[f"gtask/{t}/{k}"].ravel() for k in names]) for t in range(T)])
    has = np.stack([np.concatenate([np.full(g[f"grad/{k}"].size, g[f"has/{k}"][t]) for k in names]) for t in range(T)])
    n = gt.shape[1]
    orders = g["orders"][0].tolist()
    merged, dots, fired, norms = project64(gt, has, orders)
    assert (fired == g["fired"][0]).all()
    assert 0 < fired.sum() < T * T
    gn = np.linalg.norm(gt.astype(np.float64), axis=1)
    for i in range(T):
        for q, j in enumerate(orders[i]):
            # an fp32 dot product of n terms, on a vector that carries the rounding of up to T fp32 projections:
            # |error| <= (n + 2 T) 2^-24 sum |a||b| <= (n + 2 T) 2^-24 |pc_i| |g_j|
            bound = (n + 2 * T) * 2.0 ** -24 * norms[i, q] * gn[j]
            assert abs(dots[i, q] - g["dots"][0, i, q]) <= bound, (i, q)
            assert abs(dots[i, q]) >= 1e-2 * norms[i, q] * gn[j]  # far from a sign change
    off = 0
    for k in names:
        ref = g[f"grad/{k}"]
        mine = merged[off:off + ref.size].reshape(ref.shape)
        off += ref.size
        assert rel(ref, mine) < RTOL, k
        if k.startswith("embedding_dict."):
            assert elem_rel(ref, mine) <= 1.0, k
    # The reference's objectives are column slices of ONE concatenated prediction (model/mmoe.py:108): the slice's
    # backward seeds every head (zeros for the others), so every parameter has a gradient -- of zeros where the task does
    # not reach it -- under every objective, `shared` is all True and the merge is the mean everywhere.
    for k in names:
        assert g[f"has/{k}"].all(), k
    t_only = [k for k in names if k.startswith("tower_dnn.1.")]
    assert t_only and all(not g[f"gtask/0/{k}"].any() and g[f"gtask/1/{k}"].any() for k in t_only)
    # the coefficient form
    G = gt.astype(np.float64) @ gt.astype(np.float64).T
    c, fired_c = weights64(G, orders)
    assert (fired_c == fired).all()
    shared = has.prod(0).astype(bool)
    pc = c @ gt.astype(np.float64)
    merged_c = np.where(shared, pc.mean(0), pc.sum(0))
    assert np.abs(merged_c - merged).max() <= 1e-12 * np.abs(merged).max()


@pytest.mark.parametrize("name", PCG_CASES)
def test_fixture_losses_and_states_are_complete(name):
    g = load_golden(name)
    T = g["orders"].shape[1]
    assert g["task_losses"].shape == (3, T) and np.allclose(g["task_losses"].sum(1), g["adam_losses"], rtol=1e-12)
    assert g["X0"].shape[0] == 64 and g["y0"].shape == (64, T)
    cfg = json.loads(str(g["cfg"]))
    assert all(cfg["model_config"][k] == 0 for k in ("l2_reg_embedding", "l2_reg_dnn", "l2_reg_linear"))
    keys = [k[6:] for k in g.files if k.startswith("state/")]
    for tag in ("adam1", "adam3", "adagrad3"):
        assert [k[len(tag) + 1:] for k in g.files if k.startswith(tag + "/")] == keys
    for s in range(3):
        assert 0 < g["fired"][s].sum() < T * T  # a projection fires, a compared pair does not


def test_bad_arguments_are_rejected_without_a_gpu():
    """Every MML_ERR_ARG case of the PCGrad entry points returns before anything is launched (placeholder addresses)."""
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L
    lib = L.load()

    def seg(ld=4, banks=(0x1000, 0x2000), out=0x3000):
        arr = (L.PcgradSeg * 1)()
        for k, p in enumerate(banks):
            arr[0].bank[k] = p
        arr[0].out, arr[0].rows, arr[0].cols, arr[0].ld = out, 16, 4, ld
        return arr

    ok, big = seg(), 1 << 30
    need = lib.mml_pcgrad_workspace_bytes(ok, 1, 2)
    assert need > 0 and lib.mml_pcgrad_workspace_bytes(ok, 1, 0) == 0 and lib.mml_pcgrad_workspace_bytes(ok, 1, 9) == 0
    for T in (0, 9):
        assert lib.mml_pcgrad_gram(ok, 1, T, 0x10, 0x20, big, None) == -1
        assert lib.mml_pcgrad_combine(ok, 1, T, 0x10, None) == -1
        assert lib.mml_pcgrad_weights(0x10, 0x20, T, 0x30, None, None) == -1
    assert lib.mml_pcgrad_gram(ok, 0, 2, 0x10, 0x20, big, None) == -1                           # n < 1
    assert lib.mml_pcgrad_gram(None, 1, 2, 0x10, 0x20, big, None) == -1                         # null array
    assert lib.mml_pcgrad_gram(seg(ld=3), 1, 2, 0x10, 0x20, big, None) == -1                    # ld < cols
    assert lib.mml_pcgrad_gram(seg(banks=(None, None)), 1, 2, 0x10, 0x20, big, None) == -1      # every bank NULL
    assert lib.mml_pcgrad_combine(seg(banks=(None, None)), 1, 2, 0x10, None) == -1
    assert lib.mml_pcgrad_combine(seg(out=None), 1, 2, 0x10, None) == -1                        # null out
    assert lib.mml_pcgrad_gram(ok, 1, 2, 0x10, 0x20, need - 1, None) == -1                      # short workspace
    assert b"workspace" in lib.mml_last_error()
    assert lib.mml_pcgrad_stash(seg(out=0x1000), 1, 0, None) == -1                              # out is bank[0]
