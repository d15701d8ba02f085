"""Config loading and CSV -> model-input preparation (counterpart of the reference's utils/data_utils.py:14-111).

Runs once on the host with pandas / scikit-learn, like the reference; it is not part of the accelerated path, but it
DEFINES the X layout the kernels consume: sparse (label-encoded, contiguous ids) columns first, then the
min-max-scaled dense columns (reference :73-77), with `scene_feature` appended to the sparse list (:49-50).
Organised as a small pipeline (read -> per-dataset fixes -> encode -> schema -> split) with the same observable result
as the reference's single function; tests/test_harness.py pins layout, vocabulary sizes and the msl mask.
"""
import json
import os
import pickle

import numpy as np
import pandas as pd

from ..model.utils import DenseFeat, SparseFeat, VarLenSparseFeat, get_feature_names

__all__ = ["ctrdataset", "get_test_mask", "unserialize", "pd", "np", "os", "json"]

_LOADERS = {"json": lambda p: json.load(open(p, "r")), "npy": np.load, "ny": np.load}  # 'ny': reference typo kept


def unserialize(path):
    """json / .npy / pickle by file suffix (reference :102-111)."""
    loader = _LOADERS.get(os.path.basename(path).rsplit(".", 1)[-1])
    if loader is not None:
        return loader(path)
    with open(path, "rb") as fh:
        return pickle.load(fh)


def get_test_mask(domain_values, mask_values, num_domains):
    """float32 one-hot [N, D]: column d is (domain_values == mask_values[d]) (reference :96-100)."""
    col = np.asarray(domain_values).reshape(-1, 1)
    row = np.asarray(mask_values).reshape(1, -1)
    if row.shape[1] != num_domains:  # the reference's tiled comparison fails to broadcast in this case too
        raise ValueError(f"mask_values has {row.shape[1]} entries for num_domains = {num_domains}")
    return (col == row).astype(np.float32)


def _read_frames(dc):
    usecols = dc.get("all_columns", [])
    return (pd.read_csv(dc.get("train_dataset_path", ""), usecols=usecols),
            pd.read_csv(dc.get("test_dataset_path", ""), usecols=usecols))


def _dataset_fixes(path, columns, tr, te):
    """The per-dataset special cases the reference hard-codes on the file name (:27-39)."""
    if "kuairec" in path:
        for c in (c for c in columns if "onehot" in c):
            tr[c], te[c] = tr[c].astype(str), te[c].astype(str)
        tr = tr[tr["user_active_degree"] != "0"]
    if "iaac" in path:
        c = "predict_category_property"
        tr[c], te[c] = tr[c].astype(str), te[c].astype(str)
        te = te[:-2]
    return tr, te


def _encode(df, columns, skip, dense, stringify):
    """Contiguous ids per sparse column, [0, 1] scaling per dense column -- fitted on train + test together (:53-62)."""
    from sklearn.preprocessing import LabelEncoder, MinMaxScaler
    for c in columns:
        if c in skip:
            continue
        if stringify:
            df[c] = df[c].astype(str)
        df[c] = MinMaxScaler().fit_transform(df[[c]]).reshape(-1) if c in dense else LabelEncoder().fit_transform(df[c])
    return df


def _encode_sequences(raw, seqs, df):
    """data_config["sequence_columns"]: a cell holds `sep`-joined raw values of one vocabulary.  Returns per column
    (ids [N, maxlen] float32, lengths [N] float32 or None, vocabulary size): the LAST maxlen values of a longer
    sequence, valid ids left-packed, the rest 0.  Without `shared_with` ids are label-encoded from 1 (0 = padding) and
    the vocabulary is n_values + 1.  With it the encoder of that single-valued column is fitted on the union of both
    (the column is re-encoded here, `df` is updated in place), id 0 is then an ordinary row and the valid positions are
    given by a length column `name + "_len"`."""
    from sklearn.preprocessing import LabelEncoder
    out = {}
    for sc in seqs:
        name, maxlen, sep = sc["name"], int(sc["maxlen"]), sc.get("sep", "|")
        cells = [[v for v in str(c).split(sep) if v != ""][-maxlen:] if c == c and c is not None else []
                 for c in raw[name].tolist()]
        flat = [v for cell in cells for v in cell]
        shared = sc.get("shared_with")
        enc = LabelEncoder()
        if shared:
            single = raw[shared].astype(str)
            enc.fit(np.concatenate([single.to_numpy(), np.asarray(flat, dtype=str)]))
            df[shared] = enc.transform(single)
            base, vocab = 0, len(enc.classes_)
        else:
            enc.fit(np.asarray(flat, dtype=str))
            base, vocab = 1, len(enc.classes_) + 1
        ids = np.zeros((len(cells), maxlen), np.float32)
        codes = enc.transform(np.asarray(flat, dtype=str)) + base if flat else np.zeros(0)
        lens = np.array([len(c) for c in cells])
        pos = np.arange(maxlen)[None, :] < lens[:, None]
        ids[pos] = codes  # row-major: the cells' values in order, left-packed
        out[name] = (ids, lens.astype(np.float32) if shared else None, vocab)
    return out


def ctrdataset(config):
    """Returns (train_df, test_df, test_mask, train_model_input, test_model_input, linear_cols, dnn_cols)."""
    dc, mc = config["data_config"], config["model_config"]
    path = dc.get("train_dataset_path", "")
    columns = dc.get("all_columns", [])
    dense = dc.get("dense_columns", [])
    labels = dc.get("label_columns", ["label"])
    sparse = list(dc.get("feature_columns", []))
    scene, mask_col = dc.get("scene_feature", ""), dc.get("mask_column", "")
    scenario_mode = mc.get("task_name", "mtl") in ("msl", "mtmsl") and mask_col != ""
    if scene and scene not in sparse:
        sparse.append(scene)

    seqs = list(dc.get("sequence_columns", []))  # additive key: multi-valued columns
    tr, te = _dataset_fixes(path, columns, *_read_frames(dc))
    n_train = len(tr)
    raw = pd.concat([tr, te])
    seq_skip = {sc["name"] for sc in seqs} | {sc["shared_with"] for sc in seqs if sc.get("shared_with")}
    df = _encode(raw.copy() if seqs else raw, columns, set(labels) | set(dc.get("ignore_columns", [])) | seq_skip, dense,
                 stringify="amazon_new" in path)
    seq_data = _encode_sequences(raw, seqs, df) if seqs else {}
    # column order = X layout.  Label names may repeat (msl / mtmsl list one label once per domain): reindex() then
    # yields every duplicate, which is the reference's trick for building y with one column per head (:65-70)
    extra = [mask_col] if scenario_mode and mask_col not in sparse else []
    df = df.reindex(columns=sparse + dense + labels + extra)

    emb = mc.get("emb", 4)
    schema = [SparseFeat(c, vocabulary_size=int(df[c].max()) + 1, embedding_dim=emb) for c in sparse]
    schema += [DenseFeat(c, 1) for c in dense]
    names = get_feature_names(schema + schema)
    train, test = df[:n_train], df[n_train:]
    inputs = [{n: part[n] for n in names} for part in (train, test)]
    # multi-valued columns come after ALL single-valued ones (PepNet / APG use the scene's X column as a list position)
    for sc in seqs:
        ids, lens, vocab = seq_data[sc["name"]]
        shared = sc.get("shared_with")
        if shared:
            schema = [SparseFeat(shared, vocabulary_size=vocab, embedding_dim=emb) if f.name == shared else f
                      for f in schema]
        length_name = sc.get("length_name") or (sc["name"] + "_len" if shared else None)
        if length_name and lens is None:
            lens = (ids != 0).sum(1).astype(np.float32)  # (left-packed: the count of valid ids is the length)
        schema.append(VarLenSparseFeat(SparseFeat(sc["name"], vocabulary_size=vocab, embedding_dim=emb,
                                                  embedding_name=shared or sc["name"]),
                                       maxlen=int(sc["maxlen"]), combiner=sc.get("combiner", "mean"),
                                       length_name=length_name))
        for d, sl in zip(inputs, (slice(0, n_train), slice(n_train, None))):
            d[sc["name"]] = ids[sl]  # a 2-D [N, maxlen] entry: BaseModel._as_matrix flattens it into X
            if length_name:
                d[length_name] = lens[sl]
    test_mask = None
    if scenario_mode:
        for part, d in zip((train, test), inputs):
            if extra:
                d[mask_col] = part[mask_col]
        test_mask = get_test_mask(test[mask_col], dc.get("mask_values", []), dc.get("num_domains", 1))
    return train, test, test_mask, inputs[0], inputs[1], schema, schema
