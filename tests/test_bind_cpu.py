"""The argument builders of mmlrec_amd/bind.py against the CPU restatement of the C ABI (oracle/cabi_cpu.c), on host
tensors: mml_gather_fwd, mml_scatter_bwd and mml_gather16_fwd are called with exactly the tuples the eager wrappers and
the recorded plans pass to the HIP library, and compared bit for bit with numpy.  The shapes make every pair of
same-typed arguments distinguishable: B = 5, F = 3, E = 4, nd = 2, ldX = 8, dense_col0 = 4, ldo = 19, three different
vocabularies and a non-identity column permutation -- two swapped pointers or sizes change the result."""
import ctypes as C

import numpy as np
import pytest
import torch

B, F, E, ND = 5, 3, 4, 2
LDX, DENSE0, LDO = F + ND + 3, F + 1, F * E + ND + 5
VOCAB, COLS = [7, 11, 5], [2, 0, 1]


@pytest.fixture(scope="module")
def cpu():
    from oracle import build_fast
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, bind
    lib = C.CDLL(build_fast.build_cabi())
    for name, (res, args) in L._SIGS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib, bind


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(11)
    X = rng.standard_normal((B, LDX)).astype(np.float32)
    idx = np.stack([rng.integers(0, v, B) for v in VOCAB], 1)
    idx[0] = [v - 1 for v in VOCAB]     # the last row of every table is read: a vocabulary swap goes out of range
    idx[1:3, 1] = 9                     # a repeated row (accumulation, one touched entry), beyond the other vocabularies
    for f in range(F):
        X[:, COLS[f]] = idx[:, f]
    tables = [rng.standard_normal((v, E)).astype(np.float32) for v in VOCAB]
    # multiples of 1/8: every fp32 sum of the scatter is exact
    d_out = (rng.integers(-32, 33, (B, LDO)) / 8.0).astype(np.float32)
    return X, idx, tables, d_out


def call(lib, b):
    return getattr(lib, b.name)(*b.args, None)


def T(a):
    return torch.from_numpy(a)


def test_gather_fwd_builder(cpu, case):
    lib, bind = cpu
    X, idx, tables, _ = case
    out = np.full((B, LDO), -7.0, dtype=np.float32)
    status = np.zeros(1, dtype=np.int32)
    b = bind.gather_fwd([T(t) for t in tables], T(X), COLS, DENSE0, ND, T(out), T(status))
    assert b.name == "mml_gather_fwd" and call(lib, b) == 0 and status[0] == 0
    want = np.full((B, LDO), -7.0, dtype=np.float32)
    for f in range(F):
        want[:, f * E:(f + 1) * E] = tables[f][idx[:, f]]
    want[:, F * E:F * E + ND] = X[:, DENSE0:DENSE0 + ND]
    assert np.array_equal(out, want)


def test_gather16_fwd_builder(cpu, case):
    lib, bind = cpu
    X, idx, tables, _ = case
    out = torch.full((B, LDO), -7.0, dtype=torch.bfloat16)
    status = torch.zeros(1, dtype=torch.int32)
    b = bind.gather16_fwd([T(t) for t in tables], T(X), COLS, DENSE0, ND, out, status)
    assert b.name == "mml_gather16_fwd" and call(lib, b) == 0 and int(status) == 0
    want = torch.full((B, LDO), -7.0)
    for f in range(F):
        want[:, f * E:(f + 1) * E] = T(tables[f][idx[:, f]])
    want[:, F * E:F * E + ND] = T(X[:, DENSE0:DENSE0 + ND])
    assert torch.equal(out, want.to(torch.bfloat16))


def scatter_reference(idx, d_out):
    want = [np.zeros((v, E), dtype=np.float32) for v in VOCAB]
    for f in range(F):
        np.add.at(want[f], idx[:, f], d_out[:, f * E:(f + 1) * E])
    return want


def test_scatter_bwd_builder_without_bookkeeping(cpu, case):
    lib, bind = cpu
    X, idx, _, d_out = case
    gt = [np.zeros((v, E), dtype=np.float32) for v in VOCAB]
    status = np.zeros(1, dtype=np.int32)
    rows = bind.rows_args()
    assert rows == (None, None, None, None, 0, None)
    b = bind.scatter_bwd([T(t) for t in gt], T(X), COLS, T(d_out), rows, T(status))
    assert b.name == "mml_scatter_bwd" and call(lib, b) == 0 and status[0] == 0
    for got, want in zip(gt, scatter_reference(idx, d_out)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("loose", [False, True])
def test_scatter_bwd_builder_with_bookkeeping(cpu, case, loose):
    lib, bind = cpu
    X, idx, _, d_out = case
    gt = [np.zeros((v, E), dtype=np.float32) for v in VOCAB]
    status = np.zeros(1, dtype=np.int32)

    class Rows:  # (what optimizer.TableRows holds)
        rowbase = np.concatenate([[0], np.cumsum(VOCAB)]).tolist()
        seen = [torch.zeros((v + 31) // 32, dtype=torch.int32) for v in VOCAB]
        marks = torch.zeros(32 * sum((v + 31) // 32 for v in VOCAB), dtype=torch.uint8)
        touched = torch.full((B * F + 3,), -1, dtype=torch.int32)
        count = torch.full((B * F + 3,), -1, dtype=torch.int32)[:1]  # (room behind it: a swap with `touched` stays in bounds)

    r = Rows()
    rows = (bind.rows_args(seen=r.seen, rowbase=r.rowbase, touched=r.touched, count=r.count, marks=r.marks) if loose
            else bind.rows_args(r))
    assert rows[2:] == (r.touched.data_ptr(), r.count.data_ptr(), B * F + 3, r.marks.data_ptr())
    b = bind.scatter_bwd([T(t) for t in gt], T(X), COLS, T(d_out), rows, T(status))
    assert call(lib, b) == 0 and status[0] == 0
    for got, want in zip(gt, scatter_reference(idx, d_out)):
        assert np.array_equal(got, want)
    want_rows = sorted({r.rowbase[f] + int(i) for f in range(F) for i in idx[:, f]})
    n = int(r.count[0])
    assert n == len(want_rows)
    assert sorted(r.touched[:n].tolist()) == want_rows and bool((r.touched[n:] == -1).all())
    for f in range(F):
        bits = np.zeros(VOCAB[f], dtype=bool)
        bits[idx[:, f]] = True
        got = ((r.seen[f].numpy().view(np.uint32)[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:VOCAB[f]]
        assert np.array_equal(got.astype(bool), bits)
