"""The A/B switch of the wave-compacted loop over a warm map: read with the optimizer's other knobs (OptKnobs.from_env),
turned into mml_opt_hyper.cold_loop by one rule (optimizer.cold_loop_of) and carried by ops.make_hyper in a field that
fills the struct's former tail padding.  None of this needs a GPU."""
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


def test_knob(mod):
    O, _, _ = mod
    assert O.OptKnobs().cold_compact is True and O.OptKnobs.from_env({}).cold_compact is True
    assert O.OptKnobs.from_env({"MMLREC_OPT_COLD_COMPACT": "0"}) == O.OptKnobs(cold_compact=False)
    assert O.OptKnobs.from_env({"MMLREC_OPT_COLD_COMPACT": "1"}) == O.OptKnobs()
    assert O.OptKnobs.from_env({"MMLREC_OPT_COLD_ROWS": "0"}).cold_compact is True   # (the two switches are independent)


def test_rule_and_hyper(mod):
    O, L, ops = mod
    assert O.cold_loop_of(O.OptKnobs()) == 0
    assert O.cold_loop_of(O.OptKnobs(cold_compact=False)) == 1
    assert ops.make_hyper("adam", 0.01).cold_loop == 0
    assert ops.make_hyper("adam", 0.01, max_blocks=300, cold_loop=1).cold_loop == 1
    assert L.OptHyper().cold_loop == 0                                   # zeroed descriptors of older callers: the new loop


def test_field_sits_in_the_former_padding():
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mmlrec.h"\nint main(){printf("%zu %zu %zu\\n", '
           'sizeof(mml_opt_hyper), offsetof(mml_opt_hyper, max_blocks), offsetof(mml_opt_hyper, cold_loop));return 0;}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o",
                               os.path.join(d, "s")])
        size, off_cap, off_loop = map(int, subprocess.check_output([os.path.join(d, "s")]).split())
    assert (size, off_cap, off_loop) == (48, 40, 44)                     # 48 bytes before the field too (8-byte aligned)
    assert C.sizeof(L.OptHyper) == size and L.OptHyper.cold_loop.offset == off_loop
    assert L.OptHyper.max_blocks.offset == off_cap
