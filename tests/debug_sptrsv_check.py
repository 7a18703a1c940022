"""Run by tests/test_gpu_sptrsv.py in a child process with LHPC_LIB_PATH
pointing at the debug build (libhpc_amd/_lib_debug/liblhpc.so: device bounds
traps LHPC_DEVICE_CHECK + a synchronous check after every launch).  Valid
solves must run trap-free through the grid kernel, the chain kernel and the
value gather of lhpc_sptrsv_* — grid_rb (17-slice levels, in the chain
workgroup at chain_rows 2048), mixed and mixed_chain (grid, chain, grid) —
and give the oracle's bits.  Test infrastructure only."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import libhpc_amd as L  # noqa: E402
from tests.test_sptrsv_api import matrix, rhs, solution  # noqa: E402

assert os.path.realpath(L.LIB_PATH) == os.path.realpath(os.environ["LHPC_LIB_PATH"]), L.LIB_PATH
assert L.BUILD_FLAGS & L.BUILD_DEBUG
dev = torch.device("cuda:0")


def bits(a):
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


for name in ("grid_rb", "mixed", "mixed_chain"):
    for dt in (np.float32, np.float64):
        for upper, unit in ((False, False), (True, True)):
            rp, col, val = matrix(name, upper, dt, unit)
            want = solution(name, upper, dt, unit)
            bd = torch.from_numpy(np.array(rhs(rp.size - 1, dt))).to(dev)
            for chain_rows in (-1, 0, 64, 2048):
                with L.SpTRSVPlan(rp, col, val, upper=upper, unit_diag=unit, chain_rows=chain_rows) as P:
                    assert np.array_equal(bits(P(bd).cpu().numpy()), bits(want)), (name, dt, upper, unit, chain_rows)
                    P.set_values(torch.from_numpy(np.array(val)).to(dev))  # the gather, device and host values
                    P.set_values(np.array(val))
                    assert np.array_equal(bits(P(np.array(rhs(rp.size - 1, dt)))), bits(want))
torch.cuda.synchronize()
print("DEBUG SPTRSV OK")
