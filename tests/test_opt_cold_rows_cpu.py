"""Who may trust a table's warm map (optimizer.launch_trusts_warm_map) and who owns it (optimizer._OptState.warm,
Optimizer.warm_map / all_rows_warm): a map is born all-zero with the zero moments and nowhere else, moments that come from
outside have none, and every writer of moments that knows no map marks every row warm.  None of this needs a GPU: the
store below holds CPU tensors."""
import types

import pytest
import torch


@pytest.fixture()
def mod():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import engine as E, optimizer as O
    return O, E


def fake_optimizer(O, E, kind="adam", rows=(5, 3)):
    """An Optimizer's state and map bookkeeping over CPU tensors (no model, no library)."""
    pvals = {"embedding_dict.t%d" % i: E.PVal(torch.randn(r, 8), None, "embedding_dict.t%d" % i, is_table=True)
             for i, r in enumerate(rows)}
    pvals["dnn.w"] = E.PVal(torch.randn(4, 4), torch.zeros(4, 4), "dnn.w")
    store = types.SimpleNamespace(pvals=pvals, table_names=[n for n in pvals if n.startswith("embedding_dict.")])
    opt = O.Optimizer.__new__(O.Optimizer)
    opt.store, opt.kind = store, kind
    opt.state = O._OptState(store, kind)
    opt.warm = opt.state.warm
    return opt


def test_only_the_marked_adam_family_launch_without_regulariser_trusts_the_map(mod):
    O, _ = mod
    k = O.OptKnobs()
    for kind in ("adam", "rmsprop", "adagrad"):
        assert O.launch_trusts_warm_map(kind, True, None, k) is True
        assert O.launch_trusts_warm_map(kind, True, (), k) is True
        assert O.launch_trusts_warm_map(kind, False, None, k) is False           # unmarked / flat launch
        assert O.launch_trusts_warm_map(kind, True, (0.0, 1e-5), k) is False     # a regulariser moves every row
        assert O.launch_trusts_warm_map(kind, True, None, k, sharded=True) is False
        assert O.launch_trusts_warm_map(kind, True, None, O.OptKnobs(cold_rows=False)) is False
    assert O.launch_trusts_warm_map("sgd", True, None, k) is False


def test_knob(mod):
    O, _ = mod
    assert O.OptKnobs().cold_rows is True and O.OptKnobs.from_env({}).cold_rows is True
    assert O.OptKnobs.from_env({"MMLREC_OPT_COLD_ROWS": "0"}) == O.OptKnobs(cold_rows=False)
    assert O.OptKnobs.from_env({"MMLREC_OPT_COLD_ROWS": "1"}) == O.OptKnobs()


def test_map_is_born_zero_with_the_zero_moments(mod):
    O, E = mod
    opt = fake_optimizer(O, E)
    assert opt.warm == {}
    w = opt.warm_map("embedding_dict.t0")
    s1, s2 = opt.state["embedding_dict.t0"]
    assert w.dtype == torch.uint8 and w.shape == (5,) and int(w.max()) == 0
    assert float(s1.abs().max()) == 0.0 and float(s2.abs().max()) == 0.0
    assert opt.warm_map("embedding_dict.t0") is w                    # one map per table, kept
    opt.state["dnn.w"]
    assert "dnn.w" not in opt.warm                                   # tables only
    sgd = fake_optimizer(O, E, kind="sgd")
    assert sgd.warm_map("embedding_dict.t0") is None                 # no moments, no map


def test_loaded_moments_have_no_map(mod):
    O, E = mod
    opt = fake_optimizer(O, E)
    n = "embedding_dict.t1"
    opt.warm_map(n)
    opt.state[n] = (torch.rand(3, 8), torch.rand(3, 8))              # a load of optimizer state
    assert opt.warm_map(n) is None
    # ... also when the table had no state before, and after a deletion the next map starts with new zero moments
    opt.state["embedding_dict.t0"] = (torch.rand(5, 8), torch.rand(5, 8))
    assert opt.warm_map("embedding_dict.t0") is None
    del opt.state[n]
    assert int(opt.warm_map(n).max()) == 0 and float(opt.state[n][0].abs().max()) == 0.0


def test_writers_that_know_no_map_mark_every_row_warm(mod):
    O, E = mod
    opt = fake_optimizer(O, E)
    names = opt.store.table_names
    w0 = opt.warm_map(names[0])
    opt.all_rows_warm(names)          # (t1 had no state yet: it is made here, so that no later zero map can appear)
    assert int(w0.min()) == 1 and opt.warm_map(names[0]) is w0       # the same buffer: recorded launches see it
    assert int(opt.warm_map(names[1]).min()) == 1
    opt.state[names[1]] = (torch.rand(3, 8), torch.rand(3, 8))
    opt.all_rows_warm(names)                                         # (nothing to mark for a table without a map)
    assert opt.warm_map(names[1]) is None


def test_abi_field(mod):
    import ctypes as C
    from mmlrec_amd import _lib as L
    assert L.OptTensor.warm_rows.offset == C.sizeof(L.OptTensor) - 8 == 96
    t = (L.OptTensor * 1)()
    assert not t[0].warm_rows                                        # NULL: the update of every row
