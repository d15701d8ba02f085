"""Host-side checks of the pooled-row feature (no GPU): the C ABI of mml_pool_desc and its three entry points, the
argument checks that run before any launch, and the schema layout (X columns, dnn_input offsets) for mixed declaration
orders against the layout the reference produces."""
import ctypes
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT


def test_pool_desc_matches_the_header():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mmlrec.h"\nint main(){'
           'printf("%zu %zu %zu %d %d %d %d %d\\n", sizeof(mml_pool_desc), offsetof(mml_pool_desc, vocab), '
           'offsetof(mml_pool_desc, p_table), MML_MAX_POOLED, MML_POOL_MAX_LEN, MML_POOL_SUM, MML_POOL_MEAN, '
           'MML_POOL_MAX);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size, off_vocab, off_ptab, max_pooled, max_len, c_sum, c_mean, c_max = map(
            int, subprocess.check_output([exe]).decode().split())
    assert ctypes.sizeof(_lib.PoolDesc) == size
    assert _lib.PoolDesc.vocab.offset == off_vocab and _lib.PoolDesc.p_table.offset == off_ptab
    assert (_lib.MAX_POOLED, _lib.POOL_MAX_LEN) == (max_pooled, max_len)
    assert _lib.POOL_COMBINERS == {"sum": c_sum, "mean": c_mean, "max": c_max}


def _desc(E=8, vocab=(100,), singles=(), pooled=((0, 5, 1, 0, -1),)):
    from mmlrec_amd import _lib
    d = _lib.PoolDesc()
    d.n_tables, d.E, d.n_single, d.n_pooled = len(vocab), E, len(singles), len(pooled)
    for i, v in enumerate(vocab):
        d.vocab[i] = v
        d.table[i] = 1 << 20  # (an aligned address: never dereferenced, the calls below stop at the argument checks)
    for i, (c, t) in enumerate(singles):
        d.s_col[i], d.s_table[i] = c, t
    for i, (c0, T, comb, tb, lc) in enumerate(pooled[:_lib.MAX_POOLED]):  # (n_pooled may claim more than fit)
        d.p_col0[i], d.p_maxlen[i], d.p_combiner[i], d.p_table[i], d.p_len_col[i] = c0, T, comb, tb, lc
    return d


def test_entry_points_exist_and_reject_bad_descriptors_without_a_gpu():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib
    lib = _lib.load()
    for name in ("mml_gather_pool_fwd", "mml_gather_pool_wgmax_len", "mml_scatter_pool_bwd", "mml_index_unique_pool"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    X = out = 1 << 20
    call = lambda d, B=4, ldX=64: lib.mml_gather_pool_fwd(ctypes.byref(d), X, ldX, 0, 0, B, out, 64, None, 0, None, 0,
                                                          None, None)
    assert lib.mml_gather_pool_fwd(None, X, 64, 0, 0, 4, out, 64, None, 0, None, 0, None, None) == -1
    assert b"descriptor" in lib.mml_last_error()
    assert call(_desc(E=12)) == -1 and b"E=12" in lib.mml_last_error()
    assert call(_desc(pooled=((0, 257, 1, 0, -1),))) == -1 and b"maxlen" in lib.mml_last_error()
    assert call(_desc(pooled=((0, 0, 1, 0, -1),))) == -1
    assert call(_desc(pooled=((0, 5, 3, 0, -1),))) == -1  # unknown combiner
    assert call(_desc(pooled=((0, 5, 1, 1, -1),))) == -1  # table index out of range
    assert call(_desc(vocab=(0,))) == -1
    assert call(_desc(pooled=((0, 5, 1, 0, -1),) * 17)) == -1  # more than MML_MAX_POOLED
    assert call(_desc(), ldX=3) == -1 and b"ldX" in lib.mml_last_error()
    assert call(_desc(pooled=((0, 5, 2, 0, -1),))) == -1 and b"argmax" in lib.mml_last_error()  # max without argmax
    assert call(_desc(), B=0) == 0  # an empty batch launches nothing
    # the scatter and the index pass check the same descriptor
    assert lib.mml_scatter_pool_bwd(ctypes.byref(_desc(E=12)), X, 64, 4, out, 64, None, 0, None, None, None, None, 0,
                                    None, None, None) == -1
    assert lib.mml_index_unique_pool(ctypes.byref(_desc()), X, 64, 4, None, None, None, None, 0, None, None, None) == -1


def test_wgmax_len_counts_the_workgroups_of_every_segment():
    """Segment 0: 256 threads, one per 16-byte piece of the single-valued blocks and the dense columns; segment 1 + p:
    256 / G lane groups per workgroup, G = E / 4 lanes x the next power of two of maxlen, at most one wave; a group
    pools four samples when every position fits one pass (maxlen <= G / (E / 4)), else one."""
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib
    lib = _lib.load()
    d = _desc(E=8, vocab=(100, 50), singles=((0, 0), (1, 1)),
              pooled=((2, 5, 1, 0, -1), (7, 64, 0, 1, -1), (71, 32, 0, 1, -1)))
    B, nd = 1000, 3
    seg0 = -(-B * (2 * 2 + 1) // 256)
    seg1 = -(-B // (256 // 16 * 4))  # maxlen 5 -> 8 positions x 2 lanes, one pass: four samples per group
    seg2 = -(-B // (256 // 64))      # maxlen 64 -> one wave per sample, two passes
    seg3 = -(-B // (256 // 64 * 4))  # maxlen 32 -> one wave, one pass
    assert lib.mml_gather_pool_wgmax_len(ctypes.byref(d), nd, B) == seg0 + seg1 + seg2 + seg3
    assert lib.mml_gather_pool_wgmax_len(ctypes.byref(_desc(E=12)), nd, B) == 0


def test_ops_refuse_cpu_tensors_and_unknown_combiners():
    import torch
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import ops, _lib, functional
    with pytest.raises(ValueError):
        ops.PooledField(0, 4, "median", 0)
    with pytest.raises(_lib.MMLError):
        ops.gather_pool_fwd([torch.zeros(4, 8)], torch.zeros(2, 4), [], [ops.PooledField(0, 4, "sum", 0)])
    with pytest.raises(_lib.MMLError):
        functional.pooled_dnn_input({}, torch.zeros(2, 4), {})


def _columns(order):
    from mmlrec_amd.model import DenseFeat, SparseFeat, VarLenSparseFeat
    feats = {
        "user": SparseFeat("user", 30, embedding_dim=8),
        "item": SparseFeat("item", 40, embedding_dim=8),
        "hist": VarLenSparseFeat(SparseFeat("hist", 40, embedding_dim=8, embedding_name="item"), maxlen=6,
                                 combiner="mean", length_name="hist_len"),
        "tags": VarLenSparseFeat(SparseFeat("tags", 20, embedding_dim=8), maxlen=3, combiner="max"),
        "price": DenseFeat("price", 1),
        "age": DenseFeat("age", 1),
    }
    return [feats[n] for n in order]


def test_x_layout_and_dnn_input_offsets_for_mixed_declaration_orders():
    """X follows the declaration order (a pooled feature owns maxlen columns, its length column comes right behind
    them); dnn_input puts every single-valued block first, then the pooled blocks, then the dense columns."""
    from mmlrec_amd.model import pooled_layout
    from mmlrec_amd.model.utils import build_input_features
    cols = _columns(["user", "hist", "item", "tags", "price", "age"])
    fi = build_input_features(cols)
    assert dict(fi) == {"user": (0, 1), "hist": (1, 7), "hist_len": (7, 8), "item": (8, 9), "tags": (9, 12),
                        "price": (12, 13), "age": (13, 14)}
    lay = pooled_layout(cols)
    assert lay["table_names"] == ["user", "item", "tags"] and lay["vocab"] == [30, 40, 20] and lay["E"] == 8
    assert lay["singles"] == [(0, 0), (8, 1)]
    assert lay["pooled"] == [(1, 6, "mean", 1, 7), (9, 3, "max", 2, None)]  # hist shares the table of item
    assert (lay["dense_col0"], lay["nd"], lay["width"]) == (12, 2, 34)
    assert dict(lay["offsets"]) == {"user": (0, 8), "item": (8, 16), "hist": (16, 24), "tags": (24, 32),
                                    "price": (32, 33), "age": (33, 34)}
    # the same schema declared pooled-last: other X columns, the same dnn_input
    cols2 = _columns(["user", "item", "price", "age", "tags", "hist"])
    lay2 = pooled_layout(cols2)
    assert lay2["singles"] == [(0, 0), (1, 1)] and lay2["pooled"] == [(4, 3, "max", 2, None), (7, 6, "mean", 1, 13)]
    assert dict(lay2["offsets"])["tags"] == (16, 24) and dict(lay2["offsets"])["hist"] == (24, 32)
    assert (lay2["dense_col0"], lay2["nd"]) == (2, 2)


def test_layout_refuses_what_the_reference_would_misread():
    from mmlrec_amd.model import DenseFeat, SparseFeat, VarLenSparseFeat, pooled_layout
    item = SparseFeat("item", 40, embedding_dim=8)
    with pytest.raises(ValueError):  # a shared table with two vocabulary sizes: the reference indexes out of range
        pooled_layout([item, VarLenSparseFeat(SparseFeat("hist", 41, embedding_dim=8, embedding_name="item"), 4)])
    with pytest.raises(ValueError):
        pooled_layout([item, VarLenSparseFeat(SparseFeat("hist", 40, embedding_dim=4), 4)])
    with pytest.raises(ValueError):
        pooled_layout([item, VarLenSparseFeat(SparseFeat("hist", 40, embedding_dim=8), 4, combiner="median")])
    with pytest.raises(NotImplementedError):  # dense columns split by a sparse one
        pooled_layout([DenseFeat("a", 1), item, DenseFeat("b", 1)])


def _write_csv(d, with_seq=True):
    import pandas as pd
    train = pd.DataFrame({
        "user": [10, 11, 10, 12], "item": ["a", "b", "c", "a"], "price": [1.0, 2.0, 3.0, 4.0],
        "hist": ["a|b", "", "x|y|z|a|b", "c"], "tags": ["t1|t2", "t2", None, "t3|t1|t2|t4"],
        "label": [1, 0, 1, 0], "label2": [0, 0, 1, 1]})
    test = pd.DataFrame({
        "user": [11, 12], "item": ["b", "d"], "price": [2.5, 0.5], "hist": ["d|a", "b"], "tags": ["t4", ""],
        "label": [0, 1], "label2": [1, 0]})
    tp, sp = os.path.join(d, "train.csv"), os.path.join(d, "test.csv")
    train.to_csv(tp, index=False)
    test.to_csv(sp, index=False)
    dc = {"train_dataset_path": tp, "test_dataset_path": sp,
          "all_columns": ["user", "item", "price", "label", "label2"] + (["hist", "tags"] if with_seq else []),
          "feature_columns": ["user", "item"], "dense_columns": ["price"], "label_columns": ["label", "label2"]}
    if with_seq:
        dc["sequence_columns"] = [
            {"name": "hist", "maxlen": 3, "combiner": "mean", "sep": "|", "shared_with": "item"},
            {"name": "tags", "maxlen": 3, "combiner": "max", "sep": "|"}]
    return {"data_config": dc, "model_config": {"emb": 8, "task_name": "mtl"}}


def test_ctrdataset_sequence_columns():
    import numpy as np
    from mmlrec_amd.model import VarLenSparseFeat
    from mmlrec_amd.model.utils import build_input_features
    from mmlrec_amd.utils.data_utils import ctrdataset
    with tempfile.TemporaryDirectory() as d:
        train, test, mask, x_tr, x_te, lin, dnn = ctrdataset(_write_csv(d))
    by = {f.name: f for f in dnn}
    # the shared encoder is fitted on the union of item and the KEPT values of hist (x and y fall to the truncation):
    # a b c d z -> 0..4, one size for both features
    hist, tags = by["hist"], by["tags"]
    assert isinstance(hist, VarLenSparseFeat) and hist.embedding_name == "item" and hist.length_name == "hist_len"
    assert hist.vocabulary_size == by["item"].vocabulary_size == 5
    assert (hist.maxlen, hist.combiner, tags.maxlen, tags.combiner, tags.length_name) == (3, "mean", 3, "max", None)
    assert list(x_tr["item"]) == [0, 1, 2, 0] and list(x_te["item"]) == [1, 3]
    # truncation keeps the LAST maxlen values; valid ids are left-packed; id 0 ('a') is an ordinary row here
    assert np.array_equal(x_tr["hist"], [[0, 1, 0], [0, 0, 0], [4, 0, 1], [2, 0, 0]])
    assert np.array_equal(x_tr["hist_len"], [2, 0, 3, 1])
    assert np.array_equal(x_te["hist"], [[3, 0, 0], [1, 0, 0]]) and np.array_equal(x_te["hist_len"], [2, 1])
    # an own vocabulary: ids from 1 (0 = padding), vocabulary n_values + 1; t3 falls to the truncation: t1 t2 t4 -> 1 2 3
    assert tags.vocabulary_size == 4
    assert np.array_equal(x_tr["tags"], [[1, 2, 0], [2, 0, 0], [0, 0, 0], [1, 2, 3]])
    assert np.array_equal(x_te["tags"], [[3, 0, 0], [0, 0, 0]])
    # pooled features are declared after every single-valued and dense one; X takes the 2-D entries flattened
    assert [f.name for f in dnn] == ["user", "item", "price", "hist", "tags"]
    fi = build_input_features(dnn)
    assert dict(fi) == {"user": (0, 1), "item": (1, 2), "price": (2, 3), "hist": (3, 6), "hist_len": (6, 7),
                        "tags": (7, 10)}
    assert set(x_tr) == set(fi)


def test_config_without_sequence_columns_is_unchanged():
    """A config without the additive key gives what the commit before the key gave.  The expected frames, model inputs
    and schema below were RECORDED by running that commit's ctrdataset on this synthetic CSV (byte-level: dtypes and
    bytes of every column), not derived from the code under test; tests/test_harness.py pins the same path on the
    reference-made harness fixtures."""
    import numpy as np
    from mmlrec_amd.model import DenseFeat, SparseFeat
    from mmlrec_amd.utils.data_utils import ctrdataset
    with tempfile.TemporaryDirectory() as d:
        train, test, mask, x_tr, x_te, lin, dnn = ctrdataset(_write_csv(d, with_seq=False))
    want_tr = {"user": np.array([0, 1, 0, 2], np.int64), "item": np.array([0, 1, 2, 0], np.int64),
               "price": np.array([0.14285714285714285, 0.42857142857142855, 0.7142857142857142, 1.0], np.float64),
               "label": np.array([1, 0, 1, 0], np.int64), "label2": np.array([0, 0, 1, 1], np.int64)}
    want_te = {"user": np.array([1, 2], np.int64), "item": np.array([1, 3], np.int64),
               "price": np.array([0.5714285714285714, 0.0], np.float64),
               "label": np.array([0, 1], np.int64), "label2": np.array([1, 0], np.int64)}
    for frame, want, x in ((train, want_tr, x_tr), (test, want_te, x_te)):
        assert list(frame.columns) == list(want)
        for k, v in want.items():
            got = frame[k].to_numpy()
            assert got.dtype == v.dtype and got.tobytes() == v.tobytes(), k
        assert list(x) == ["user", "item", "price"]
        for k in x:
            got = np.asarray(x[k])
            assert got.dtype == want[k].dtype and got.tobytes() == want[k].tobytes(), k
    assert mask is None
    assert lin == dnn == [SparseFeat("user", 3, embedding_dim=8), SparseFeat("item", 4, embedding_dim=8),
                          DenseFeat("price", 1)]


@pytest.mark.parametrize("name", ["pooled_mmoe_mtl", "pooled_pepnet_mtmsl", "pooled_mmoe_e16", "pooled_sharedbottom_sum"])
def test_committed_fixtures_meet_the_criteria_against_their_float64_tensors(name):
    """The generator's assertion, repeated on the committed files: the reference's own fp32 tensors meet every criterion
    of tests/test_pooled_models_gpu.py against its float64 tensors with at least 10x headroom, so the criteria are the
    reference's own with room to spare."""
    import numpy as np
    from conftest import load_golden
    g = load_golden(name)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < (1 << 20)

    def rel(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)

    def elem_rel(a, b, floor=1e-5):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return (np.abs(a - b) / (1e-4 * np.abs(b) + floor * max(np.abs(b).max(), 1e-30))).max()

    assert rel(g["dnn_input"], g["dnn_input64"]) < 1e-5
    assert rel(g["y_pred"], g["y_pred64"]) < 1e-5  # (no dropout, no BatchNorm: the eval and the training forward agree)
    assert abs(float(g["loss"]) - float(g["loss64"])) / float(g["loss64"]) < 1e-5
    keys = [k[7:] for k in g.files if k.startswith("grad64/")]
    assert keys and any(k.startswith("embedding_dict.") for k in keys)
    for k in keys:
        assert rel(g["grad/" + k], g["grad64/" + k]) < 1e-5, k
        if k.startswith("embedding_dict."):
            assert elem_rel(g["grad/" + k], g["grad64/" + k]) <= 0.1, k
