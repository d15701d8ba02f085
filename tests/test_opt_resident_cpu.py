"""What the resident grid of the dense table update and the per-step constants need off the GPU: the new descriptor's
layout, the knobs and the rule that turns them into mml_opt_hyper.cold_loop, and the entry a step's call list starts with."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT


@pytest.fixture()
def mod():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, optimizer as O, ops
    return O, L, ops


def test_struct_sizes_and_offsets(mod):
    _, L, _ = mod
    fields = ["sizeof(mml_opt_step_consts)", "offsetof(mml_opt_step_consts, step)",
              "offsetof(mml_opt_step_consts, step_size)", "offsetof(mml_opt_step_consts, inv_bc2s)",
              "sizeof(mml_opt_hyper)", "offsetof(mml_opt_hyper, step_dev)", "offsetof(mml_opt_hyper, max_blocks)",
              "offsetof(mml_opt_hyper, cold_loop)", "sizeof(mml_opt_tensor)"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mmlrec.h"\nint main(){' +
           "".join('printf("%%zu ", %s);' % f for f in fields) + "return 0;}")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o",
                               os.path.join(d, "s")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "s")]).split()))
    assert got == [16, 0, 4, 8, 48, 8, 40, 44, 104]
    S, H = L.OptStepConsts, L.OptHyper
    assert [C.sizeof(S), S.step.offset, S.step_size.offset, S.inv_bc2s.offset] == got[:4]
    assert [C.sizeof(H), H.step_dev.offset, H.max_blocks.offset, H.cold_loop.offset] == got[4:8]
    assert C.sizeof(L.OptTensor) == got[8]
    # 32 descriptors, the hyper, both prefix tables and the constants' pointer travel by value in 4 KB of kernel arguments
    assert 32 * got[8] + 8 + got[4] + 33 * 8 + 33 * 4 + 4 + 8 <= 4096


def test_exports(mod):
    _, L, _ = mod
    lib = L.load()
    assert {"mml_opt_step_begin", "mml_opt_step_unbind"} <= set(L.EXPORTS)
    assert lib.mml_opt_step_begin(None, 1, None, None, None) == -1      # (refused before anything touches a GPU)
    h = L.OptHyper()
    h.kind = L.OPT_KINDS["adam"]
    assert lib.mml_opt_step_begin(None, 1, C.byref(h), None, None) == -1 and b"counter" in lib.mml_last_error()
    assert lib.mml_opt_step_unbind(None) == 0                           # (nothing bound: nothing to do)


def test_knobs(mod):
    O, _, _ = mod
    k = O.OptKnobs()
    assert (k.resident, k.step_consts) == (1, True) and O.OptKnobs.from_env({}) == k
    assert O.OptKnobs.from_env({"MMLREC_OPT_RESIDENT": "0"}) == O.OptKnobs(resident=0)
    assert O.OptKnobs.from_env({"MMLREC_OPT_RESIDENT": "2"}) == O.OptKnobs(resident=2)
    assert O.OptKnobs.from_env({"MMLREC_OPT_STEP_CONSTS": "0"}) == O.OptKnobs(step_consts=False)
    assert O.OptKnobs.from_env({"MMLREC_OPT_COLD_COMPACT": "0"}).resident == 1   # (independent switches)


def test_cold_loop_rule(mod):
    O, _, ops = mod
    assert O.cold_loop_of(O.OptKnobs()) == 0                            # the compacted loop on the chip-sized grid
    assert O.cold_loop_of(O.OptKnobs(resident=0)) == 2                  # ... on each tensor's workgroups
    assert O.cold_loop_of(O.OptKnobs(resident=2)) == 3                  # ... on the halved grid
    for r in (0, 1, 2):                                                 # the byte loop knows one grid only
        assert O.cold_loop_of(O.OptKnobs(cold_compact=False, resident=r)) == 1
    assert ops.make_hyper("adam", 0.01).cold_loop == 0
    assert ops.make_hyper("adam", 0.01, cold_loop=2).cold_loop == 2


def test_pre_entry(mod):
    """One entry either way: the combined launch when a constants buffer is bound, the plain counter otherwise."""
    O, L, ops = mod
    lib = L.load()
    h = ops.make_hyper("adam", 0.01)
    fn, args = O.step_pre_entry(lib, 4096, 4096 + 16, h)
    assert fn is lib.mml_opt_step_begin or fn.__name__ == "mml_opt_step_begin"
    assert args[:2] == (4096, 1) and args[3] == 4096 + 16 and len(args) == 4
    fn, args = O.step_pre_entry(lib, 4096, None, h)
    assert fn.__name__ == "mml_counter_update" and args == (4096, 1, 0)


def test_optimizer_pre_list(mod, monkeypatch):
    """Optimizer.calls_split starts the step with exactly one entry: mml_opt_step_begin on the optimizer's own counter and
    buffer (one allocation, the buffer 16 bytes in and 16-byte aligned), or -- MMLREC_OPT_STEP_CONSTS=0 -- the plain bump."""
    import torch
    O, L, ops = mod

    class Store:
        device = torch.device("cpu")
        table_names = []
        pvals = {}

        class model:
            regularization_weight = []

            @staticmethod
            def named_parameters():
                return []

    class Plan:
        ops = []

        def __init__(self):
            self.keep = []

    opt = O.Optimizer(Store(), "adam", 0.01, table_update="dense_exact")
    assert opt.step_consts.data_ptr() == opt.step_dev.data_ptr() + 16 and opt.step_consts.data_ptr() % 16 == 0
    assert opt.step_dev.numel() == 1 and opt.step_consts.numel() * opt.step_consts.element_size() == 16
    monkeypatch.delenv("MMLREC_OPT_STEP_CONSTS", raising=False)
    pre = opt.calls_split(Plan())["pre"]
    assert len(pre) == 1 and pre[0][0].__name__ == "mml_opt_step_begin"
    assert pre[0][1][0] == opt.step_dev.data_ptr() and pre[0][1][3] == opt.step_consts.data_ptr()
    monkeypatch.setenv("MMLREC_OPT_STEP_CONSTS", "0")
    pre = opt.calls_split(Plan())["pre"]
    assert len(pre) == 1 and pre[0][0].__name__ == "mml_counter_update"
    assert pre[0][1] == (opt.step_dev.data_ptr(), 1, 0)
