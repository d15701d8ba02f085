"""mml_opt_tensor grew by the deferred totals of the deterministic scatter (acc64 / acc_amax / acc_shift, appended): the
ctypes mirror keeps the C layout, OptLaunch still fits a kernel-argument block, and the CPU restatement of
mml_opt_step_dense (oracle/cabi_cpu.c, compiled against the same header) gives the Adam step it gave with the new
fields at zero."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from conftest import ROOT


def test_opt_tensor_mirror_matches_the_header_and_fits_a_launch():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mmlrec.h"\nint main(){printf("%zu %zu %zu %zu %d %d %d\\n", '
           'sizeof(mml_opt_tensor), offsetof(mml_opt_tensor, acc64), offsetof(mml_opt_tensor, acc_shift), '
           'sizeof(mml_opt_hyper), MML_SCATTER_DET_CLEAR_MARKS, MML_SCATTER_DET_AMAX_SUPPLIED, '
           'MML_SCATTER_DET_DEFER_TOTALS);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o",
                               os.path.join(d, "s")])
        size, off_acc, off_shift, hyper, f1, f2, f4 = map(int, subprocess.check_output([os.path.join(d, "s")]).split())
    assert C.sizeof(L.OptTensor) == size
    assert L.OptTensor.acc64.offset == off_acc and L.OptTensor.acc_shift.offset == off_shift
    assert (f1, f2, f4) == (L.SCATTER_DET_CLEAR_MARKS, L.SCATTER_DET_AMAX_SUPPLIED, L.SCATTER_DET_DEFER_TOTALS)
    # csrc/optim.hip's OptLaunch (passed by value): the tensors, the hyper-parameters, n / variant / prop and the two
    # prefix tables -- under the 4 KB of a kernel-argument block
    launch = L.MAX_OPT_TENSORS * size + hyper + 3 * 4 + (L.MAX_OPT_TENSORS + 1) * (8 + 4)
    assert launch + 16 <= 4096, launch


def test_cpu_adam_step_is_unchanged_with_the_new_fields_at_zero():
    from oracle import build_fast
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L
    lib = C.CDLL(build_fast.build_cabi())
    lib.mml_opt_step_dense.restype, lib.mml_opt_step_dense.argtypes = L._SIGS["mml_opt_step_dense"]
    rng = np.random.default_rng(0)
    n, lr, b1, b2, eps, step = 64, 0.005, 0.9, 0.999, 1e-8, 3
    p, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    m, v = (0.1 * rng.standard_normal(n)).astype(np.float32), rng.random(n).astype(np.float32)
    p0, m0, v0 = p.copy(), m.copy(), v.copy()
    t = (L.OptTensor * 1)()
    t[0].param, t[0].grad, t[0].state1, t[0].state2, t[0].n = p.ctypes.data, g.ctypes.data, m.ctypes.data, v.ctypes.data, n
    assert not t[0].acc64 and not t[0].acc_amax and t[0].acc_shift == 0
    h = L.OptHyper()
    h.kind, h.step, h.lr, h.beta1, h.beta2, h.eps, h.alpha = L.OPT_ADAM, step, lr, b1, b2, eps, 0.99
    assert lib.mml_opt_step_dense(t, 1, C.byref(h), None) == 0
    f32 = np.float32
    m1 = f32(b1) * m0 + (f32(1) - f32(b1)) * g
    v1 = f32(b2) * v0 + (f32(1) - f32(b2)) * g * g
    denom = np.sqrt(v1) / f32(np.sqrt(1.0 - float(f32(b2)) ** step)) + f32(eps)
    want = p0 - f32(lr / (1.0 - float(f32(b1)) ** step)) * (m1 / denom)
    assert np.allclose(m, m1, rtol=1e-6, atol=0) and np.allclose(v, v1, rtol=1e-6, atol=0)
    assert np.abs(p - want).max() <= 2e-6 * np.abs(want).max()
    assert float(np.abs(p - p0).max()) > 0
