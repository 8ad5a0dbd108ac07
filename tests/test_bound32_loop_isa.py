"""The address form of k_bound32_sums' block loop, read off the gfx950 code of the library as built (csrc/kernels_bound32.hip, DESIGN.md
section 5.22.2).  The form is steered by empty asm statements and one scheduling barrier; a compiler that stops honouring them would cost
time, not correctness, and no device test would see it.  So the loop is pinned here: in each of the 48 instantiations the basic block
that holds the matrix instructions has no 64-bit vector add or move, every global load in it takes a scalar base with a 32-bit lane
offset, and it still holds its 4 KS matrix instructions and KS + 2 (+ 1 with the w . r sum) loads.  CPU only: llvm-objdump."""
import os
import re

import pytest

from bogp import _lib
from tests.support import isa_lint

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(isa_lint.LLVM_BIN, "llvm-objdump")), reason="needs llvm-objdump of the ROCm toolchain")

NAME = re.compile(r"k_bound32_sumsILi(\d)ELi(\d)ELb([01])E")
SADDR = re.compile(r"^v\S*, v\d+, s\[\d+:\d+\]")  # destination, ONE 32-bit offset register, a scalar pair


def loop_block(insns):
    """the instructions from the loop's first matrix instruction back to the nearest branch target or branch, and on to its last"""
    idx = [i for i, (_, mn, _) in enumerate(insns) if mn.startswith("v_mfma")]
    lo = idx[0]
    while lo > 0 and not insns[lo - 1][1].startswith(("s_cbranch", "s_branch", "s_barrier")):
        lo -= 1
    return insns[lo : idx[-1] + 1]


@pytest.fixture(scope="module")
def kernels():
    found = {}
    for text in isa_lint.disassemble_library(_lib.LIB_PATH):
        for name, insns in isa_lint.parse_functions(text).items():
            m = NAME.search(name)
            if m:
                found[tuple(int(g) for g in m.groups())] = insns
    return found


def test_all_48_instantiations_are_in_the_library(kernels):
    assert sorted(kernels) == sorted((k, ks, wd) for k in (0, 2, 3) for ks in range(1, 9) for wd in (0, 1))


def test_no_vector_address_arithmetic_between_the_loads_and_the_matrix_chain(kernels):
    bad = []
    for (k, ks, wd), insns in sorted(kernels.items()):
        blk = loop_block(insns)
        ops = [mn for _, mn, _ in blk]
        loads = [(mn, args) for _, mn, args in blk if mn.startswith(("global_load", "flat_load"))]
        wide = [mn for mn in ops if mn.startswith(("v_lshl_add_u64", "v_mov_b64", "v_add_co", "v_addc_co", "v_mad_u64", "v_mad_i64"))]
        if wide:
            bad.append("<%d, %d, %d>: %s in the block" % (k, ks, wd, sorted(set(wide))))
        if sum(mn.startswith("v_mfma") for mn in ops) != 4 * ks:
            bad.append("<%d, %d, %d>: %d matrix instructions in the block, not %d" % (k, ks, wd, sum(mn.startswith("v_mfma") for mn in ops), 4 * ks))
        if len(loads) != ks + 2 + wd:
            bad.append("<%d, %d, %d>: %d loads in front of the chain, not %d" % (k, ks, wd, len(loads), ks + 2 + wd))
        for mn, args in loads:
            if not (mn.startswith("global_load") and SADDR.match(args)):
                bad.append("<%d, %d, %d>: %s %s is not the scalar-base form" % (k, ks, wd, mn, args))
    assert not bad, "\n".join(bad)
