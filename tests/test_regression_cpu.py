"""Regression heads, the parts that need no GPU: the head-kind constants of include/mmlrec.h against _lib, struct sizes
against the C compiler, compile()'s validation of losses and metrics, the metric column rule on plain arrays, and the
fixtures of tests/golden/make_golden_regression.py."""
import ctypes
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT, load_golden

REG_CASES = ["reg_mmoe_mtl", "reg_ple", "reg_pepnet_mtmsl", "reg_star_msl", "reg_sharedbottom", "reg_mmoe_seconds"]
# sizeof() of the four descriptor structs before `pad_` became `kind` (measured with gcc on the parent's header)
SIZES = {"mml_head_desc": 136, "mml_head_group": 1192, "mml_tower_head_desc": 192, "mml_tower_head_group": 1608}


def header_defines():
    txt = open(os.path.join(ROOT, "include", "mmlrec.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(MML_HEAD_[A-Z_]+)\s+(\d+)\s", txt)}


def test_head_kind_constants_agree_with_the_header():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L
    d = header_defines()
    assert d == {"MML_HEAD_OUT_SIGMOID": L.HEAD_OUT_SIGMOID, "MML_HEAD_OUT_IDENTITY": L.HEAD_OUT_IDENTITY,
                 "MML_HEAD_LOSS_BCE": L.HEAD_LOSS_BCE, "MML_HEAD_LOSS_MSE": L.HEAD_LOSS_MSE,
                 "MML_HEAD_LOSS_MAE": L.HEAD_LOSS_MAE}
    assert (d["MML_HEAD_OUT_SIGMOID"], d["MML_HEAD_OUT_IDENTITY"]) == (0, 1)
    assert (d["MML_HEAD_LOSS_BCE"], d["MML_HEAD_LOSS_MSE"], d["MML_HEAD_LOSS_MAE"]) == (0, 1, 2)
    assert L.head_kind() == 0 and L.head_kind(L.HEAD_OUT_IDENTITY, L.HEAD_LOSS_MAE) == 0x201
    # the macro of the header packs the same word
    src = ('#include <stdio.h>\n#include "mmlrec.h"\nint main(){printf("%d %d %d\\n", '
           'MML_HEAD_KIND(MML_HEAD_OUT_IDENTITY, MML_HEAD_LOSS_MAE), MML_HEAD_KIND_OUT(0x201), MML_HEAD_KIND_LOSS(0x201));'
           'return 0;}')
    with tempfile.TemporaryDirectory() as t:
        c, exe = os.path.join(t, "k.c"), os.path.join(t, "k")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        assert subprocess.check_output([exe]).decode().split() == ["513", "1", "2"]


def test_struct_sizes_are_unchanged_and_kind_sits_where_the_padding_was():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L
    mirrors = {"mml_head_desc": L.HeadDesc, "mml_head_group": L.HeadGroup, "mml_tower_head_desc": L.TowerHeadDesc,
               "mml_tower_head_group": L.TowerHeadGroup}
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "mmlrec.h"\nint main(){' + "".join(
        f'printf("{n} %zu\\n", sizeof({n}));' for n in mirrors) + \
        'printf("hk %zu\\n", offsetof(mml_head_desc, kind));printf("tk %zu\\n", offsetof(mml_tower_head_desc, kind));return 0;}'
    with tempfile.TemporaryDirectory() as t:
        c, exe = os.path.join(t, "s.c"), os.path.join(t, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split()
    got = dict(zip(out[0::2], map(int, out[1::2])))
    for n, cls in mirrors.items():
        assert got[n] == SIZES[n] == ctypes.sizeof(cls), (n, got[n], SIZES[n], ctypes.sizeof(cls))
    assert got["hk"] == SIZES["mml_head_desc"] - 4 == L.HeadDesc.kind.offset
    assert got["tk"] == SIZES["mml_tower_head_desc"] - 4 == L.TowerHeadDesc.kind.offset


def cpu_model(task_types, cls="MMOE", task_name="mtl", **data_kw):
    import mmlrec_amd  # noqa: F401
    import torch
    from mmlrec_amd import model as M
    from mmlrec_amd.model import DenseFeat, SparseFeat
    cfg = json.loads(str(load_golden("mmoe_kuairec")["cfg"]))
    cfg["model_config"].update(emb=8, task_name=task_name, task_names=["a", "b"], task_types=list(task_types))
    cfg["data_config"].update(data_kw)
    cols = [SparseFeat("user", 50, embedding_dim=8), SparseFeat("scene", 2, embedding_dim=8), DenseFeat("price", 1)]
    torch.manual_seed(0)
    return getattr(M, cls)(cols, device="cpu", config=cfg)


def test_compile_validates_losses_and_metrics():
    m = cpu_model(["binary", "regression"])
    assert [type(o).__name__ for o in m.out] == ["PredictionLayer", "PredictionLayer"]  # the reference's module tree
    assert sorted(k for k in m.state_dict() if k.startswith("out.")) == ["out.0.bias", "out.1.bias"]
    from mmlrec_amd import _lib as L
    assert m._head_kind(0) == 0 and m._head_kind(1) == L.head_kind(L.HEAD_OUT_IDENTITY, L.HEAD_LOSS_MSE)  # before compile
    m.compile("adam", ["binary_crossentropy", "mae"], ["auc", "mse", "acc", "logloss"])
    assert m.loss_func == ["binary_crossentropy", "mae"]
    assert m._head_kind(1) == L.head_kind(L.HEAD_OUT_IDENTITY, L.HEAD_LOSS_MAE)
    assert m.metric_cols == {"auc": [0], "mse": [1], "acc": [0], "logloss": [0]}
    m.compile("adam", ["mse", "mse"], ["mse"])  # sigmoid + MSE
    assert m._head_kind(0) == L.head_kind(L.HEAD_OUT_SIGMOID, L.HEAD_LOSS_MSE)
    with pytest.raises(ValueError):
        m.compile("adam", ["binary_crossentropy", "binary_crossentropy"], ["auc"])
    with pytest.raises(ValueError):
        m.compile("adam", "binary_crossentropy", ["auc"])  # one name for every task: the regression task refuses it
    with pytest.raises(NotImplementedError):
        m.compile("adam", ["binary_crossentropy", "huber"], ["auc"])
    with pytest.raises(ValueError):
        m.compile("adam", ["mse"], ["auc"])
    m = cpu_model(["regression", "regression"])
    with pytest.raises(ValueError):
        m.compile("adam", ["mse", "mae"], ["auc"])
    m.compile("adam", "mse", ["mse"])
    assert m.metric_cols == {"mse": [0, 1]}
    m = cpu_model(["binary", "binary"])
    m.compile("adam", ["binary_crossentropy"] * 2, ["auc", "acc", "mse"])
    assert m.metric_cols == {"auc": None, "acc": None, "mse": None}  # all binary: as before
    with pytest.raises(ValueError):
        cpu_model(["binary", "multiclass"])
    for cls in ("ESMM", "ESCM", "AITM"):
        with pytest.raises((NotImplementedError, ValueError)):
            cpu_model(["binary", "regression"], cls=cls)
        m = cpu_model(["binary", "binary"], cls=cls)
        with pytest.raises(NotImplementedError):
            m.compile("adam", ["binary_crossentropy", "mse"], ["auc"])
        m.compile("adam", ["binary_crossentropy"] * 2, ["auc"])


def test_metric_column_rule_on_plain_arrays():
    from sklearn.metrics import mean_squared_error, roc_auc_score
    rng = np.random.default_rng(0)
    N = 200
    m = cpu_model(["binary", "regression"])
    m.compile("adam", ["binary_crossentropy", "mse"], ["auc", "mse", "acc"])
    y = np.stack([rng.random(N) < 0.4, rng.random(N) * 3], 1).astype(np.float64)
    p = np.stack([rng.random(N), rng.random(N) * 3], 1)
    assert m._metric(m.metrics["auc"], y, p, m.metric_cols["auc"]) == roc_auc_score(y[:, 0], p[:, 0])
    assert m._metric(m.metrics["mse"], y, p, m.metric_cols["mse"]) == mean_squared_error(y[:, 1], p[:, 1])
    assert m._metric(m.metrics["acc"], y, p, m.metric_cols["acc"]) == float(((p[:, 0] > 0.5) == (y[:, 0] > 0.5)).mean())
    # without the rule (the reference's way) the mixed label matrix has no AUC at all
    assert np.isnan(m._metric(m.metrics["auc"], y, p))
    # mtmsl: two label groups of D = 2 domains each; the first binary, the second a regression
    m = cpu_model(["binary", "binary", "regression", "regression"], task_name="mtmsl",
                  label_columns=["l", "l", "w", "w"], num_domains=2, mask_values=[0, 1], mask_column="scene",
                  scene_feature="scene")
    m.compile("adam", ["binary_crossentropy"] * 2 + ["mse"] * 2, ["auc", "mse"])
    assert m.metric_cols == {"auc": [0], "mse": [1]}
    y4 = np.stack([y[:, 0], y[:, 0], y[:, 1], y[:, 1]], 1)
    p4 = np.stack([p[:, 0] * 0.3, p[:, 0] * 0.7, p[:, 1] * 0.5, p[:, 1] * 0.5], 1)
    assert abs(m._metric(m.metrics["auc"], y4, p4, [0]) - roc_auc_score(y[:, 0], p[:, 0])) < 1e-12
    assert abs(m._metric(m.metrics["mse"], y4, p4, [1]) - mean_squared_error(y[:, 1], p[:, 1])) < 1e-12
    # msl: one summed column
    m = cpu_model(["regression", "regression"], task_name="msl", label_columns=["w", "w"], num_domains=2,
                  mask_values=[0, 1], mask_column="scene", scene_feature="scene")
    m.compile("adam", ["mse", "mse"], ["mse"])
    assert m.metric_cols == {"mse": [0]}
    with pytest.raises(ValueError):
        m.compile("adam", ["mse", "mse"], ["auc"])


@pytest.mark.parametrize("name", REG_CASES)
def test_fixture_sanity(name):
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    assert os.path.getsize(path) < 1024 * 1024
    g = load_golden(name)
    cfg = json.loads(str(g["cfg"]))
    types, losses = cfg["model_config"]["task_types"], cfg["optim_config"]["loss"]
    T = g["y0"].shape[1]
    assert len(types) == len(losses) == T == g["y_pred"].shape[1] == g["y_pred64"].shape[1]
    for k in ("X0", "X1", "X2", "y0", "y1", "y2", "init_y_pred", "y_pred", "y_pred64", "loss", "loss64", "headroom"):
        assert k in g.files, k
    assert any(k.startswith("state/") for k in g.files) and any(k.startswith("grad64/") for k in g.files)
    assert {k[7:] for k in g.files if k.startswith("grad64/")} == {k[5:] for k in g.files if k.startswith("grad/")}
    opts = [k[:-7] for k in g.files if k.endswith("_losses")]
    assert opts and all(len(g[o + "_losses"]) == 3 for o in opts)
    for o in opts:
        assert any(k.startswith(f"{o}1/") for k in g.files) and any(k.startswith(f"{o}3/") for k in g.files)
    if cfg["model_config"]["task_name"] in ("msl", "mtmsl"):
        assert "mask0" in g.files and "y_pred_masked" in g.files
    for k in g.files:  # arrays and JSON strings only
        assert g[k].dtype.kind in "fiuU", (k, g[k].dtype)
    # what the generator measured: the reference's fp32 tensors against its float64 twin with 10x headroom under 1e-4,
    # MAE samples 100x clear of the fp32-float64 prediction distance, continuous labels without repeats
    h = json.loads(str(g["headroom"]))
    assert h["y"] < 1e-5 and h["loss"] < 1e-5 and h["grad"] < 1e-5 and h["table_elem"] <= 0.1, h
    assert h["labels_distinct"] is True
    assert ("mae" in losses) == (h["mae_margin"] is not None)
    if h["mae_margin"] is not None:
        assert h["mae_margin"] > 100.0
    for t in range(T):
        for i in range(3):
            col = g[f"y{i}"][:, t]
            if types[t] == "regression":
                assert len(np.unique(col)) == len(col) and not np.all(col == np.round(col))
            else:
                assert set(np.unique(col)) <= {0.0, 1.0}
    if name == "reg_mmoe_seconds":  # watch time in seconds: labels in the hundreds
        assert 30.0 < g["y0"][:, 1].min() and g["y0"][:, 1].max() > 300.0
