"""Every argument builder of mmlrec_amd/bind.py against the ctypes signature table (_lib._SIGS), and the two builders the
CPU restatement of the C ABI (oracle/cabi_cpu.c) implements, run through it.

(a) Each public builder is called with host tensors of distinguishable shapes -- B = 5 rows, widths 3, 4 and 7, every row
pitch wider than its width and no two alike -- and its tuple is held to the entry point's argtypes: the arity, a pointer
slot holds None, a ctypes array, a byref or the address of one of the tensors given, an integer slot holds a Python int
that is none of those addresses, a float slot a float.  That catches a missing or doubled argument and a pointer, size or
float in the wrong kind of slot; the ORDER within a run of one kind is the business of the kernel tests, which spell the
calls by hand (tests/test_model_kernels_gpu.py, tests/test_kernels_gpu.py, tests/test_row_kernels_gpu.py,
tests/test_pcgrad_gpu.py) and of tests/test_bind_model_gpu.py, which holds the builders to them on the device.
(b) bind.dropout and bind.amax_reset on host memory through libmmlrec_cpu.so, bit for bit against the oracle's mask
(the reference tests/test_cabi_cpu.py uses for mml_dropout): distinct pitches, row0 != 0, accumulate 0 and 1, a seed and
a site wider than the 64 / 32 bits the call takes."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

B, W3, W4, W7 = 5, 3, 4, 7
HELPERS = {"ld", "ptr_array", "rows_args"}  # public names of bind.py that build no Bound


@pytest.fixture(scope="module")
def mods():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, bind
    return L, bind


class Mk:
    """Host tensors for one builder call; remembers every address it hands out."""

    def __init__(self):
        self.addr, self.keep, self.n = set(), [], 0

    def _reg(self, t):
        self.addr.add(t.data_ptr())
        self.keep.append(t)
        return t

    def mat(self, cols, rows=B, dtype=torch.float32):
        self.n += 1  # (pitches 25, 26, 27, ...: wider than every width used here, all different)
        assert cols <= 24
        return self._reg(torch.zeros(rows, 24 + self.n, dtype=dtype)[:, :cols])

    def vec(self, n, dtype=torch.float32):
        return self._reg(torch.zeros(n, dtype=dtype))

    def tables(self, E=W4):
        return [self.mat(E, rows=v) for v in (7, 11, 6)]

    def rows(self, bind):
        return bind.rows_args(seen=[self.vec(1, torch.int32) for _ in range(3)], rowbase=[0, 7, 18, 24],
                              touched=self.vec(9, torch.int32), count=self.vec(1, torch.int32),
                              marks=self.vec(96, torch.uint8))


def _cases(L, bind):
    """name -> callable(Mk) -> Bound, for every public builder."""
    cols = [2, 0, 1]
    i32, u8, i64 = torch.int32, torch.uint8, torch.int64
    seg = (L.PcgradSeg * 2)()
    return {
        # ---- row family
        "gather_fwd": lambda m: bind.gather_fwd(m.tables(), m.mat(W7), cols, 4, 2, m.mat(14), m.vec(1, i32)),
        "gather16_fwd": lambda m: bind.gather16_fwd(m.tables(), m.mat(W7), cols, 4, 2, m.mat(14, dtype=torch.bfloat16),
                                                    m.vec(1, i32)),
        "gather_fwd_wgmax": lambda m: bind.gather_fwd_wgmax(m.tables(), m.mat(W7), cols, 4, 2, m.mat(14), m.mat(6, rows=1), 6,
                                                            m.vec(1, i32)),
        "gather_fwd_mark": lambda m: bind.gather_fwd_mark(m.tables(), m.mat(W7), cols, 4, 2, m.mat(14), m.vec(96, u8),
                                                          m.vec(1, i32)),
        "gather_fwd_idx32": lambda m: bind.gather_fwd_idx32(m.tables(), m.mat(W3, dtype=i32), m.mat(2), m.mat(14),
                                                            m.vec(1, i32)),
        "gather_pool_fwd": lambda m: bind.gather_pool_fwd(L.PoolDesc(), m.mat(W7), 4, 2, m.mat(14), m.mat(W4, dtype=u8),
                                                          m.mat(6, rows=1), 6, m.vec(1, i32)),
        "scatter_bwd": lambda m: bind.scatter_bwd(m.tables(), m.mat(W7), cols, m.mat(12), m.rows(bind), m.vec(1, i32)),
        "scatter_bwd_det": lambda m: bind.scatter_bwd_det(m.tables(), m.mat(W7), cols, m.mat(12),
                                                          [m.mat(W4, rows=v, dtype=i64) for v in (7, 11, 6)],
                                                          m.vec(8, i32), m.vec(96, u8), 5, m.vec(1, i32)),
        "scatter_bwd_idx32": lambda m: bind.scatter_bwd_idx32(m.tables(), m.mat(W3, dtype=i32), m.mat(12), m.rows(bind),
                                                              m.vec(1, i32)),
        "scatter_pool_bwd": lambda m: bind.scatter_pool_bwd(L.PoolDesc(), m.mat(W7), m.mat(12), m.mat(W4, dtype=u8),
                                                            m.rows(bind), m.vec(1, i32)),
        "scatter_pool_bwd_det": lambda m: bind.scatter_pool_bwd_det(L.PoolDesc(), m.mat(W7), m.mat(12), m.mat(W4, dtype=u8),
                                                                    [m.mat(W4, rows=v, dtype=i64) for v in (7, 11, 6)],
                                                                    m.vec(8, i32), m.vec(96, u8), 5, m.vec(1, i32)),
        "index_unique": lambda m: bind.index_unique([7, 11, 6], cols, W4, m.mat(W7), m.rows(bind), m.vec(1, i32)),
        "index_unique_pool": lambda m: bind.index_unique_pool(L.PoolDesc(), m.mat(W7), m.rows(bind), m.vec(1, i32)),
        "rows_compact": lambda m: bind.rows_compact([7, 11, 6], m.rows(bind)),
        "opt_step_rows": lambda m: bind.opt_step_rows(m.tables(), m.tables(), m.tables(), None, m.rows(bind), L.OptHyper(),
                                                      last=[m.vec(v, i32) for v in (7, 11, 6)]),
        "opt_catchup_rows": lambda m: bind.opt_catchup_rows(m.tables(), m.tables(), None, [m.vec(v, i32) for v in (7, 11, 6)],
                                                            m.rows(bind), L.OptHyper()),
        # ---- model layer
        "bn_fwd": lambda m: bind.bn_fwd(m.mat(W7), m.vec(W7), m.vec(W7), m.vec(W7), m.vec(W7), m.vec(1, i64), m.vec(W7),
                                        m.vec(W7), m.mat(W7), 1, True, 1e-5, 0.1, m.vec(64, u8)),
        "bn_bwd": lambda m: bind.bn_bwd(m.mat(W7), m.mat(W7), m.vec(W7), m.vec(W7), m.vec(W7), m.mat(W7), m.vec(W7), m.vec(W7),
                                        True, m.vec(64, u8)),
        "domain_bn_update": lambda m: bind.domain_bn_update(m.mat(W7), m.mat(W3), m.mat(W7, rows=W3), m.mat(W7, rows=W3), 0.99),
        "domain_bn_eval": lambda m: bind.domain_bn_eval(m.mat(W7), m.mat(W3), m.mat(W7, rows=W3), m.mat(W7, rows=W3),
                                                        m.mat(W7), 1e-5),
        "dropout": lambda m: bind.dropout(m.mat(W7), m.mat(W7), 0.25, (1 << 70) + 5, (1 << 40) + 3, m.vec(1, i32), 0, True, 11),
        "apg_features_fwd": lambda m: bind.apg_features_fwd(m.mat(W3), m.mat(W4), m.mat(W3 * W4 + W7), W3, W4),
        "apg_features_bwd": lambda m: bind.apg_features_bwd(m.mat(W3 * W4 + W3), m.mat(W4), m.mat(W3), W3, W4, True),
        "apg_weights": lambda m: bind.apg_weights(m.mat(W4, rows=9), m.vec(9), m.mat(W4, rows=W3), m.mat(W3, rows=19), W3, W4,
                                                  1, (1, 0, 1)),
        "snr_gate_weights_fwd": lambda m: bind.snr_gate_weights_fwd(m.vec(6), m.vec(6), m.vec(72), m.vec(72), 6, 12, 1, 0.9,
                                                                    -0.1, 1.1),
        "snr_gate_weights_bwd": lambda m: bind.snr_gate_weights_bwd(m.vec(72), m.vec(72), m.vec(6), m.vec(6), None, m.vec(6),
                                                                    0, True, 6, 12, 1, 0.9, -0.1, 1.1, m.vec(6)),
        "esmm_combine": lambda m: bind.esmm_combine(m.mat(2), m.mat(2), None, m.mat(2), m.mat(2), m.vec(1), B),
        "escm_combine": lambda m: bind.escm_combine(m.mat(2), None, m.mat(W3), m.mat(W3), m.mat(2), None, B, 0.1, 1),
        "ew_mul": lambda m: bind.ew_mul(m.vec(35), m.vec(35), m.vec(35)),
        "ew_mul_bwd": lambda m: bind.ew_mul_bwd(m.vec(35), m.vec(35), m.vec(35), m.vec(35), None, True, False),
        "ew_mul_bwd_act": lambda m: bind.ew_mul_bwd_act(m.vec(35), m.vec(35), m.vec(35), m.vec(35), m.vec(35), 0, 0, 1, 2),
        "ew_add_n": lambda m: bind.ew_add_n([m.vec(35), m.vec(35), m.vec(35)], m.mat(W7), n=B * 12),
        "act_bwd": lambda m: bind.act_bwd(m.mat(W7), m.mat(W7), m.mat(W7), 1, n=B * 12),
        "copy2d": lambda m: bind.copy2d(m.mat(W4), m.mat(W4), True),
        "copy_flat": lambda m: bind.copy_flat(m.vec(35), m.vec(35), False),
        "pcgrad_gram": lambda m: bind.pcgrad_gram(seg, 2, 3, m.vec(9, torch.float64), m.vec(256, u8)),
        "pcgrad_weights": lambda m: bind.pcgrad_weights(m.vec(9, torch.float64), m.vec(9, i32), 3, m.vec(6), m.vec(9, i32)),
        "pcgrad_combine": lambda m: bind.pcgrad_combine(seg, 2, 3, m.vec(6)),
        "pcgrad_stash": lambda m: bind.pcgrad_stash(seg, 2, True),
        "counter_update": lambda m: bind.counter_update(m.vec(1, i32), 1, False),
        "amax_reset": lambda m: bind.amax_reset(m.mat(8, rows=4, dtype=i32), 3),
    }


def test_every_public_builder_has_a_case(mods):
    L, bind = mods
    public = {n for n, f in inspect.getmembers(bind, inspect.isfunction)
              if not n.startswith("_") and f.__module__ == bind.__name__} - HELPERS
    assert public == set(_cases(L, bind))


def _is_byref(a):
    return hasattr(a, "_obj") and isinstance(a._obj, C.Structure)


def _misfits(L, bind, name, build):
    """What is wrong with one builder's tuple, as text ([] = it fits its signature)."""
    m = Mk()
    b = build(m)
    if not isinstance(b, bind.Bound) or b.name not in L._SIGS:
        return ["%s: no Bound of a known entry point" % name]
    argtypes = L._SIGS[b.name][1]
    if len(b.args) + 1 != len(argtypes) or argtypes[-1] is not L.fp:  # (the last slot: the stream the consumer appends)
        return ["%s: %d arguments for the %d of %s" % (name, len(b.args), len(argtypes) - 1, b.name)]
    bad = []
    for k, (a, t) in enumerate(zip(b.args, argtypes)):
        if t in (L.i32, L.i64, C.c_uint32, C.c_uint64):
            bits = 8 * C.sizeof(t)
            lo, hi = (0, 1 << bits) if t in (C.c_uint32, C.c_uint64) else (-(1 << bits - 1), 1 << bits - 1)
            fits = type(a) is int and a not in m.addr and lo <= a < hi
        elif t is C.c_float:
            fits = type(a) is float
        elif t is L.fp:
            fits = a is None or isinstance(a, C.Array) or _is_byref(a) or (type(a) is int and a in m.addr)
        else:  # a typed pointer: an array of that element type, a byref of that structure, or null
            fits = a is None or (isinstance(a, C.Array) and a._type_ is t._type_) or \
                (_is_byref(a) and type(a._obj) is t._type_)
        if not fits:
            bad.append("%s: argument %d of %s is %r for a %s slot" % (name, k, b.name, a, t.__name__))
    return bad


def test_every_builder_fits_its_signature(mods):
    L, bind = mods
    bad = [msg for name, build in sorted(_cases(L, bind).items()) for msg in _misfits(L, bind, name, build)]
    assert not bad, "\n".join(bad)


# ---- (b) through the CPU restatement of the C ABI ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu(mods):
    from oracle import build_fast
    L, bind = mods
    lib = C.CDLL(build_fast.build_cabi())
    for name, (res, args) in L._SIGS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib, bind


@pytest.mark.parametrize("accumulate", [0, 1])
def test_dropout_builder_is_the_oracle_mask(cpu, accumulate):
    lib, bind = cpu
    from oracle import mmlrec_oracle as orc
    rng = np.random.default_rng(5)
    rows, cols, p, step, row0 = B, W7, 0.3, 5, 11
    seed, site = 0xfeedfacecafebeef, 0x9e3779b9
    x = rng.standard_normal((rows, cols + 2)).astype(np.float32)          # pitch 9
    prior = rng.standard_normal((rows, cols + 4)).astype(np.float32)      # pitch 11
    out = prior.copy()
    sd = torch.tensor([step], dtype=torch.int32)
    b = bind.dropout(torch.from_numpy(x)[:, :cols], torch.from_numpy(out)[:, :cols], p, seed + (3 << 64), site + (7 << 32),
                     sd, 99, accumulate, row0)                             # (step_dev given: `step` = 99 is not read)
    assert b.name == "mml_dropout" and getattr(lib, b.name)(*b.args, None) == 0
    want = x[:, :cols] * orc.dropout_scale(rows, cols, p, seed, step, site, row0=row0)
    if accumulate:
        want = want + prior[:, :cols]
    assert np.array_equal(out[:, :cols], want.astype(np.float32))
    assert np.array_equal(out[:, cols:], prior[:, cols:])                  # the padding columns are not written
    assert not np.array_equal(want, x[:, :cols] * np.float32(1 / (1 - p)))  # (some element is dropped)


def test_amax_reset_builder(cpu):
    lib, bind = cpu
    pool = torch.full((4, 8), 7, dtype=torch.int32)
    b = bind.amax_reset(pool, 3)
    assert b.name == "mml_amax_reset" and getattr(lib, b.name)(*b.args, None) == 0
    assert not bool(pool[:3].any()) and bool((pool[3] == 7).all())
