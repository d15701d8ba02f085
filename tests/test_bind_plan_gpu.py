"""A recorded plan entry and the eager wrapper launch the same thing: GatherOp and PooledGatherOp record their forward and
backward on a bare Plan (engine.Plan.bound over mmlrec_amd/bind.py), the entries are run, and every result is compared
bit for bit with the ops.* call on the same inputs.  The last test does the same for the model-layer ops that have an eager
twin (DropoutOp, CopyColsOp, PAddOp), at B = 5.

Schema: 2 single-valued fields and 2 pooled fields (maxlen 3; one "sum", one "max"), the "sum" field sharing its table
with a single field; E = 8, B = 257 (more than one block, no multiple of a tile), one dense column, 37 .. 61 rows per table.
The upstream gradients are integer multiples of 1/8 with |g| <= 4, so every fp32 sum of the atomic scatter is exact and
the tables compare bit for bit whatever the order of the atomics; touched lists compare as sorted sets."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

E_, B, ND = 8, 257, 1
VOCAB = [37, 53, 61]                             # tables 0, 1, 2
SINGLES = [(0, 0), (1, 1)]                       # (X column, table)
POOLED = [(2, 3, "sum", 1, None), (5, 3, "max", 2, None)]  # (first X column, maxlen, combiner, table, length column)
DENSE0 = 8


def _padded(rows, n, dev, dtype=torch.float32):
    return torch.empty(rows, (n + 3) // 4 * 4, dtype=dtype, device=dev)[:, :n]


@pytest.fixture(scope="module")
def env():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import engine as E, ops, optimizer as O
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    X = torch.zeros(B, DENSE0 + ND)
    X[:, 0] = torch.randint(0, VOCAB[0], (B,), generator=g)
    X[:, 1] = torch.randint(0, VOCAB[1], (B,), generator=g)
    for col0, maxlen, _, t, _ in POOLED:         # id 0 = an empty position (mask mode); some samples are all empty
        ids = torch.randint(1, VOCAB[t], (B, maxlen), generator=g)
        ids[torch.rand(B, maxlen, generator=g) < 0.3] = 0
        X[:, col0:col0 + maxlen] = ids
    X[:, DENSE0] = torch.randn(B, generator=g)
    tables = [torch.randn(v, E_, generator=g).to(dev) for v in VOCAB]
    K_pool, K_single = (len(SINGLES) + len(POOLED)) * E_ + ND, len(SINGLES) * E_ + ND
    grad = (torch.randint(-32, 33, (B, K_pool), generator=g) / 8.0)
    return dict(E=E, ops=ops, O=O, dev=dev, X=X.to(dev), tables=tables, grad=grad.to(dev), K_pool=K_pool, K_single=K_single)


def _plan(env, wgmax=True):
    plan = env["E"].Plan(env["dev"], B, True)
    plan.knobs = dataclasses.replace(plan.knobs, gather_wgmax=wgmax)
    return plan


def _pvals(env, which):
    E = env["E"]
    return [E.PVal(env["tables"][t], torch.zeros_like(env["tables"][t]), f"t{t}", is_table=True) for t in which]


def _single_op(env, sparse_rows=None):
    E, dev = env["E"], env["dev"]
    pv = _pvals(env, [t for _, t in SINGLES])
    out = E.Val(_padded(B, env["K_single"], dev), name="dnn_input")
    out.grad = _padded(B, env["K_single"], dev)
    out.grad.copy_(env["grad"][:, :env["K_single"]])
    return E.GatherOp(pv, env["X"], [c for c, _ in SINGLES], DENSE0, ND, out, sparse_rows=sparse_rows), pv, out


def _pooled_op(env, sparse_rows=None):
    E, dev = env["E"], env["dev"]
    pv = _pvals(env, range(len(VOCAB)))
    out = E.Val(_padded(B, env["K_pool"], dev), name="dnn_input")
    out.grad = _padded(B, env["K_pool"], dev)
    out.grad.copy_(env["grad"])
    return E.PooledGatherOp(pv, env["X"], SINGLES, POOLED, DENSE0, ND, out, sparse_rows=sparse_rows), pv, out


def _fields(env):
    return [env["ops"].PooledField(*pf) for pf in POOLED]


def _same_rows(a, b):
    """Two TableRows hold the same row set: count, touched list as a sorted set, `seen` bitmaps."""
    na, nb = int(a.count.item()), int(b.count.item())
    assert na == nb and na > 0
    assert torch.equal(torch.sort(a.touched[:na]).values, torch.sort(b.touched[:nb]).values)
    assert all(torch.equal(x, y) for x, y in zip(a.seen, b.seen))


@pytest.mark.parametrize("wgmax", [True, False])
def test_gather_forward_entry_is_the_eager_call(env, wgmax):
    E, ops = env["E"], env["ops"]
    plan = _plan(env, wgmax)
    op, pv, out = _single_op(env)
    calls = op.fwd_calls(plan)
    want_fn = "mml_gather_fwd_wgmax" if wgmax and plan.amax_pool is not None else "mml_gather_fwd"
    assert [c[0].__name__ for c in calls] == [want_fn]
    E.Plan._run(calls)
    tabs, cols = [t.data for t in pv], [c for c, _ in SINGLES]
    if want_fn == "mml_gather_fwd_wgmax":
        ref, wg = ops.gather_fwd_wgmax(tabs, env["X"], cols, DENSE0, ND, out=_padded(B, env["K_single"], env["dev"]))
        assert torch.equal(out.amax_src[:, :calls[0][1][-2]], wg[:, :calls[0][1][-2]])
    else:
        ref = ops.gather_fwd(tabs, env["X"], cols, DENSE0, ND)
    torch.cuda.synchronize()
    assert torch.equal(out.buf, ref) and int(plan.status.item()) == 0


@pytest.mark.parametrize("wgmax", [True, False])
def test_pooled_gather_forward_entry_is_the_eager_call(env, wgmax):
    E, ops = env["E"], env["ops"]
    plan = _plan(env, wgmax)
    op, pv, out = _pooled_op(env)
    calls = op.fwd_calls(plan)
    assert [c[0].__name__ for c in calls] == ["mml_gather_pool_fwd"]
    E.Plan._run(calls)
    takes_wg = wgmax and plan.amax_pool is not None
    ref, argmax, wg = ops.gather_pool_fwd([t.data for t in pv], env["X"], SINGLES, _fields(env), DENSE0, ND, wgmax=takes_wg)
    torch.cuda.synchronize()
    assert torch.equal(out.buf, ref) and torch.equal(op.argmax, argmax) and int(plan.status.item()) == 0
    if takes_wg:
        n = calls[0][1][-2]
        assert n > 0 and torch.equal(out.amax_src[:, :n], wg[:, :n])


def test_scatter_backward_entries_are_the_eager_calls(env):
    """Atomic mode with touched-row bookkeeping, then deterministic mode."""
    E, ops, O, dev = env["E"], env["ops"], env["O"], env["dev"]
    vocab = [VOCAB[t] for _, t in SINGLES]
    cols = [c for c, _ in SINGLES]
    rows, rows2 = (O.TableRows(vocab, dev, B * len(SINGLES)) for _ in range(2))
    plan = _plan(env)
    op, pv, out = _single_op(env, sparse_rows=rows)
    calls = op.bwd_calls(plan)
    assert [c[0].__name__ for c in calls] == ["mml_scatter_bwd"] and calls[0][2]["tail"]
    E.Plan._run(calls)
    gt = [torch.zeros_like(t.data) for t in pv]
    ops.scatter_bwd(gt, env["X"], cols, out.grad, seen=rows2.seen, rowbase=rows2.rowbase, touched=rows2.touched,
                    touched_count=rows2.count, marks=rows2.marks, status=plan.status)
    torch.cuda.synchronize()
    assert all(torch.equal(t.grad, g) for t, g in zip(pv, gt)) and any(bool(g.any()) for g in gt)
    _same_rows(rows, rows2)
    assert int(plan.status.item()) == 0

    def det():
        return dict(acc64=[torch.zeros(v, E_, dtype=torch.int64, device=dev) for v in vocab],
                    marks=torch.zeros(ops.marks_bytes(vocab), dtype=torch.uint8, device=dev), slot=ops.amax_slots(1, dev)[0])

    op, pv, out = _single_op(env)
    op.deterministic = det()
    calls = op.bwd_calls(plan)
    assert [c[0].__name__ for c in calls] == ["mml_scatter_bwd_det"]
    assert calls[0][2]["det_flags"] == E.L.SCATTER_DET_CLEAR_MARKS
    E.Plan._run(calls)
    d2 = det()
    gt_det = [torch.zeros_like(t.data) for t in pv]
    ops.scatter_bwd_det(gt_det, env["X"], cols, out.grad, d2["acc64"], d2["marks"], amax_slot=d2["slot"], status=plan.status)
    torch.cuda.synchronize()
    assert all(torch.equal(t.grad, g) for t, g in zip(pv, gt_det))
    assert all(torch.equal(a, b) for a, b in zip(gt, gt_det))  # (exact sums: the two modes agree as well)
    assert not any(bool(a.any()) for a in op.deterministic["acc64"]) and not bool(op.deterministic["marks"].any())


def test_pooled_scatter_backward_entries_are_the_eager_calls(env):
    E, ops, O, dev = env["E"], env["ops"], env["O"], env["dev"]
    lookups = len(SINGLES) + sum(pf[1] for pf in POOLED)
    rows, rows2 = (O.TableRows(VOCAB, dev, B * lookups) for _ in range(2))
    plan = _plan(env)
    op, pv, out = _pooled_op(env, sparse_rows=rows)
    E.Plan._run(op.fwd_calls(plan))              # (the "max" field's backward reads the forward's argmax)
    calls = op.bwd_calls(plan)
    assert [c[0].__name__ for c in calls] == ["mml_scatter_pool_bwd"] and calls[0][2]["tail"]
    E.Plan._run(calls)
    gt = [torch.zeros_like(t.data) for t in pv]
    ops.scatter_pool_bwd(gt, env["X"], SINGLES, _fields(env), out.grad, argmax=op.argmax, seen=rows2.seen,
                         rowbase=rows2.rowbase, touched=rows2.touched, touched_count=rows2.count, marks=rows2.marks,
                         status=plan.status)
    torch.cuda.synchronize()
    assert all(torch.equal(t.grad, g) for t, g in zip(pv, gt)) and all(bool(g.any()) for g in gt)
    _same_rows(rows, rows2)

    # the index pre-pass of lazy_exact lists the same rows without gradients
    rows3, rows4 = (O.TableRows(VOCAB, dev, B * lookups) for _ in range(2))
    E.Plan._run(op.unique_calls(plan, rows3))
    ops.index_unique_pool(VOCAB, E_, env["X"], SINGLES, _fields(env), rows4.seen, rows4.rowbase, rows4.touched, rows4.count,
                          status=plan.status, marks=rows4.marks)
    torch.cuda.synchronize()
    _same_rows(rows3, rows4)
    _same_rows(rows3, rows)

    def det():
        return dict(acc64=[torch.zeros(v, E_, dtype=torch.int64, device=dev) for v in VOCAB],
                    marks=torch.zeros(ops.marks_bytes(VOCAB), dtype=torch.uint8, device=dev), slot=ops.amax_slots(1, dev)[0])

    argmax = op.argmax
    op, pv, out = _pooled_op(env)
    op.argmax, op.deterministic = argmax, det()
    calls = op.bwd_calls(plan)
    assert [c[0].__name__ for c in calls] == ["mml_scatter_pool_bwd_det"]
    assert calls[0][2]["det_flags"] == E.L.SCATTER_DET_CLEAR_MARKS
    E.Plan._run(calls)
    d2 = det()
    gt_det = [torch.zeros_like(t.data) for t in pv]
    ops.scatter_pool_bwd_det(gt_det, env["X"], SINGLES, _fields(env), out.grad, d2["acc64"], d2["marks"], argmax=argmax,
                             amax_slot=d2["slot"], status=plan.status)
    torch.cuda.synchronize()
    assert all(torch.equal(t.grad, g) for t, g in zip(pv, gt_det))
    assert all(torch.equal(a, b) for a, b in zip(gt, gt_det))
    assert int(plan.status.item()) == 0


def test_dropout_copy_and_add_entries_are_the_eager_calls(env):
    """The model-layer ops whose eager twin exists, at B = 5 with a pitch of its own per buffer: DropoutOp (forward and
    backward), CopyColsOp, PAddOp (forward: mml_ew_add_n, backward: the flat mml_copy2d)."""
    E, ops, dev = env["E"], env["ops"], env["dev"]
    Bs, n, p, seed, site = 5, 7, 0.3, (1 << 64) + 0xfeedfacecafebeef, (1 << 32) + 0x9e3779b9
    g = torch.Generator().manual_seed(3)

    def mat(cols, ld, c0=0):
        return torch.randn(Bs, ld, generator=g).to(dev)[:, c0:c0 + cols]

    plan = E.Plan(dev, Bs, True)
    plan.step_dev, plan.row0 = torch.tensor([5], dtype=torch.int32, device=dev), 3
    x, y = E.Val(mat(n, 9), name="x"), E.Val(mat(n, 11), name="y")
    op = E.DropoutOp(x, y, p, seed, site)
    x.consumers.append(op)
    calls = op.fwd_calls(plan)
    assert [c[0].__name__ for c in calls] == ["mml_dropout"] and calls[0][1][8] < (1 << 64) and calls[0][1][9] < (1 << 32)
    E.Plan._run(calls)
    ref = mat(n, 13)
    ops.dropout(x.buf, ref, p, seed, site, step=99, step_dev=plan.step_dev, row0=3)
    assert torch.equal(y.buf, ref) and bool((ref == 0).any()) and bool((ref != 0).any())
    y.grad = mat(n, 10)
    calls = op.bwd_calls(plan)
    assert [c[0].__name__ for c in calls] == ["mml_dropout"] and calls[0][1][-1] == 0
    E.Plan._run(calls)
    ops.dropout(y.grad, ref, p, seed, site, step_dev=plan.step_dev, row0=3)
    assert torch.equal(x.grad, ref)

    src, dst, ref = mat(4, 9, 2), mat(4, 12, 3), mat(4, 6, 1)
    calls = E.CopyColsOp(src, dst).fwd_calls(plan)
    assert [c[0].__name__ for c in calls] == ["mml_copy2d"] and calls[0][2] == {}
    E.Plan._run(calls)
    ops.copy2d(src, ref)
    assert torch.equal(dst, ref) and torch.equal(dst, src)

    ins = [E.PVal(torch.randn(n, generator=g).to(dev), torch.full((n,), 7.0, device=dev), f"b{i}") for i in range(3)]
    out = E.PVal(torch.zeros(n, device=dev), torch.randn(n, generator=g).to(dev), "b_eff")
    add = E.PAddOp(ins, out)
    E.Plan._run(add.fwd_calls(plan))
    ref = torch.zeros(n, device=dev)
    ops.ew_add_n([q.data for q in ins], ref)
    assert torch.equal(out.data, ref) and bool(ref.any())
    out.written = 1
    calls = add.bwd_calls(plan)
    assert [c[0].__name__ for c in calls] == ["mml_copy2d"] * 3
    assert all(c[2] == dict(kernel="copy2d_kernel", side=True) for c in calls)
    E.Plan._run(calls)
    ref = torch.full((1, n), 7.0, device=dev)
    ops.copy2d(out.grad.view(1, n), ref)
    assert all(torch.equal(q.grad, ref[0]) for q in ins) and torch.equal(ref[0], out.grad)
