"""functional.pooled_dnn_input -- the public, differentiable form of the pooled-row kernels -- against the reference's
own chain of torch ops (nn.Embedding over the id columns, the mask from `ids != 0` or from the length column,
SequencePoolingLayer's sum / mean / max, the concatenation of combined_dnn_input) restated here in float64 on the CPU.

Criteria, as in tests/test_pooled_rows_gpu.py: single-valued blocks, dense columns and max blocks bit-exact; sum / mean
blocks within the worst-case bound of an fp32 summation in any order; table gradients rel < 1e-4 and elem_rel <= 1
against float64, with a table shared by a single-valued and a pooled feature accumulating both."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-4
U = 2.0 ** -24


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def elem_rel(a, b, floor=1e-5):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    return (np.abs(a - b) / (RTOL * np.abs(b) + floor * scale)).max()


def schema(E):
    from mmlrec_amd.model import DenseFeat, SparseFeat, VarLenSparseFeat
    return [SparseFeat("user", 300, embedding_dim=E),
            VarLenSparseFeat(SparseFeat("hist", 500, embedding_dim=E, embedding_name="item"), maxlen=20,
                             combiner="mean", length_name="hist_len"),
            SparseFeat("item", 500, embedding_dim=E),
            VarLenSparseFeat(SparseFeat("tags", 60, embedding_dim=E), maxlen=5, combiner="max"),
            VarLenSparseFeat(SparseFeat("cats", 90, embedding_dim=E), maxlen=12, combiner="sum"),
            DenseFeat("price", 1)]


def make_x(cols, fi, B, rng):
    from mmlrec_amd.model import SparseFeat, VarLenSparseFeat
    X = np.zeros((B, max(e for _, e in fi.values())), np.float32)
    for f in cols:
        a, b = fi[f.name]
        if isinstance(f, SparseFeat):
            X[:, a] = rng.integers(0, f.vocabulary_size, B)
        elif isinstance(f, VarLenSparseFeat):
            V, T = f.vocabulary_size, f.maxlen
            ids = np.minimum(rng.zipf(1.3, (B, T)), V - 1)
            lo = 1 if f.combiner == "max" else 0  # an all-padded max sample's reference gradient depends on tie-breaking
            n = rng.integers(lo, T + 1, B)
            if f.length_name is None:
                ids[np.arange(T)[None, :] >= n[:, None]] = 0
                hole = (rng.random(B) < 0.25) & (n > 2)
                ids[hole, 1] = 0  # a padded slot in the middle
            else:
                X[:, fi[f.length_name][0]] = n
            ids[0, 0], ids[1, 0] = 1, V - 1
            X[:, a:b] = ids
        else:
            X[:, a] = rng.standard_normal(B)
    return X


def reference64(cols, fi, tables64, X):
    """The reference's forward in float64 (model/utils.py:258-326, :449-463, :520-533; model/basemodel.py:461-487)."""
    from mmlrec_amd.model import DenseFeat, SparseFeat, VarLenSparseFeat
    Xt = torch.from_numpy(X)
    blocks, bounds = [], []
    for f in [c for c in cols if isinstance(c, SparseFeat)]:
        blocks.append(tables64[f.embedding_name][Xt[:, fi[f.name][0]].long()])
        bounds.append(torch.zeros_like(blocks[-1]))
    for f in [c for c in cols if isinstance(c, VarLenSparseFeat)]:
        a, b = fi[f.name]
        ids = Xt[:, a:b].long()
        emb = tables64[f.embedding_name][ids]  # [B, T, E]
        if f.length_name is None:
            mask = (ids != 0)
        else:
            ln = Xt[:, fi[f.length_name][0]].long()
            mask = torch.arange(f.maxlen)[None, :] < ln[:, None]
        n = mask.sum(1, keepdim=True)
        m = mask.unsqueeze(2).double()
        if f.combiner == "max":
            h = emb - ((1 - m) * 1e9)
            blocks.append(h.max(dim=1)[0])
            bounds.append(torch.zeros_like(blocks[-1]))
            continue
        s = (emb * m).sum(1)
        bound = f.maxlen * U * (emb.detach().abs() * m).sum(1)
        if f.combiner == "mean":
            s = s / (n.float() + torch.tensor(1e-8)).double()
            bound = bound / n.clamp(min=1) + U * s.detach().abs()
        blocks.append(s)
        bounds.append(bound)
    de = [c for c in cols if isinstance(c, DenseFeat)]
    if de:
        blocks.append(Xt[:, fi[de[0].name][0]:fi[de[-1].name][1]].double())
        bounds.append(torch.zeros_like(blocks[-1]))
    return torch.cat(blocks, 1), torch.cat(bounds, 1)


@pytest.mark.parametrize("E", [4, 8, 16])
@pytest.mark.parametrize("B", [64, 1000])
def test_pooled_dnn_input_forward_and_autograd(E, B):
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import functional
    from mmlrec_amd.model import pooled_layout
    from mmlrec_amd.model.utils import build_input_features, create_embedding_matrix
    torch.manual_seed(5)
    rng = np.random.default_rng(11 * E + B)
    cols = schema(E)
    fi = build_input_features(cols)
    lay = pooled_layout(cols, fi)
    emb = create_embedding_matrix(cols, init_std=0.1, device="cuda:0")
    assert sorted(emb.keys()) == ["cats", "item", "tags", "user"]  # hist uses the table of item
    X = make_x(cols, fi, B, rng)
    w = torch.from_numpy(rng.standard_normal((B, lay["width"])).astype(np.float32))
    out = functional.pooled_dnn_input(emb, torch.from_numpy(X).cuda(), lay)
    (out * w.cuda()).sum().backward()
    t64 = {k: v.weight.detach().cpu().double().requires_grad_(True) for k, v in emb.items()}
    ref, bound = reference64(cols, fi, t64, X)
    (ref * w.double()).sum().backward()
    got = out.detach().cpu().numpy()
    exact = (bound == 0).numpy()
    r = ref.detach().numpy()
    assert np.array_equal(got[exact], r.astype(np.float32)[exact])  # copies and max blocks: bit-exact
    err = np.abs(got.astype(np.float64) - r)
    print(f"[pooled functional] E={E} B={B}: max err/bound = "
          f"{float((err[~exact] / np.maximum(bound.numpy()[~exact], 1e-300)).max()):.3g}")
    assert np.all(err <= bound.numpy())
    for k in emb.keys():
        g, g64 = emb[k].weight.grad.cpu().numpy(), t64[k].grad.numpy()
        print(f"[pooled functional] E={E} B={B} {k}: rel={rel(g, g64):.3g} elem_rel={elem_rel(g, g64):.3g}")
        assert rel(g, g64) < RTOL and elem_rel(g, g64) <= 1.0, k
        assert not g[(g64 == 0).all(1)].view(np.uint32).any(), k  # rows without a valid lookup: bitwise 0


def test_out_of_range_id_raises_like_nn_embedding():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import functional
    from mmlrec_amd.model import pooled_layout
    from mmlrec_amd.model.utils import build_input_features, create_embedding_matrix
    cols = schema(8)
    fi = build_input_features(cols)
    emb = create_embedding_matrix(cols, device="cuda:0")
    X = make_x(cols, fi, 64, np.random.default_rng(0))
    X[3, fi["cats"][0]] = 90  # == vocabulary_size at a valid position
    X[3, fi["cats"][0] + 1] = 1
    from mmlrec_amd import ops
    status = ops.new_status(torch.device("cuda:0"))
    functional.pooled_dnn_input(emb, torch.from_numpy(X).cuda(), pooled_layout(cols, fi), status=status)
    with pytest.raises(IndexError):
        ops.check_status(status, "pooled_dnn_input")
