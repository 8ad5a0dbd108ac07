"""The one remaining instrument of the contraction, the -DCONTRACT_D_TRACE build of k_contract16d (tools/contract_d_trace.py, DESIGN.md
section 10 item 1), is defined in no product build, so nothing else would notice it rotting: kernels_posterior.hip and bogp_api_sweep.hip
must compile for gfx950 with the switch, and the host object must define the export the tool binds.  CPU only: hipcc cross-compiles."""
import os
import subprocess

import pytest

from bogp import _lib
from tests.support import isa_lint

CSRC = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(os.path.join(isa_lint.LLVM_BIN, "llvm-objdump"))),
                                reason="needs the ROCm toolchain (hipcc, llvm-objdump)")


def test_the_trace_build_compiles_and_exports_its_read_back(tmp_path):
    objs = {}
    procs = []
    for src in ("kernels_posterior.hip", "bogp_api_sweep.hip"):
        objs[src] = str(tmp_path / (src + ".o"))
        procs.append(subprocess.Popen([HIPCC, "-DCONTRACT_D_TRACE", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-result",
                                       "-I/opt/rocm/include", "-c", os.path.join(CSRC, src), "-o", objs[src]],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))  # fmt: skip
    for p in procs:
        out = p.communicate()[0]
        assert p.returncode == 0, out[-4000:]
    nm = os.path.join(isa_lint.LLVM_BIN, "llvm-nm")
    syms = subprocess.run([nm if os.path.exists(nm) else "nm", "--defined-only", objs["bogp_api_sweep.hip"]], check=True, capture_output=True, text=True).stdout
    assert any(ln.split()[-1] == "bogp_debug_contract_trace" for ln in syms.splitlines() if ln.split()), "the trace build no longer exports bogp_debug_contract_trace"
    syms = subprocess.run([nm if os.path.exists(nm) else "nm", "--defined-only", objs["kernels_posterior.hip"]], check=True, capture_output=True, text=True).stdout
    assert "debug_contract_trace" in syms, "kernels_posterior.hip no longer defines bogp::debug_contract_trace under the switch"
