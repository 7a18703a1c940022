"""Run by tests/test_gpu_set_values.py in a child process with LHPC_LIB_PATH
pointing at the debug build (libhpc_amd/_lib_debug/liblhpc.so: device bounds
traps LHPC_DEVICE_CHECK + a synchronous check after every launch).  Valid
updates must run trap-free through lhpc_spmv_plan_set_values' kernels — the
XTILE value transpose (perm / iperm, fp32 / fp64, row parts) and the SELL
row-offset scan and scatter — and leave the plan equal to a fresh one.
Test infrastructure only."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import libhpc_amd as L  # noqa: E402
from tests.test_gpu_spmv import _csr_from_lengths  # noqa: E402

assert os.path.realpath(L.LIB_PATH) == os.path.realpath(os.environ["LHPC_LIB_PATH"]), L.LIB_PATH
assert L.BUILD_FLAGS & L.BUILD_DEBUG
dev = torch.device("cuda:0")
rng = np.random.default_rng(0xDB)


def check(rp, col, n_cols, dt, flags, opts=None):
    v0, v1 = (rng.uniform(-1, 1, col.size).astype(dt) for _ in range(2))
    xd = torch.from_numpy(rng.uniform(-1, 1, n_cols).astype(dt)).to(dev)
    with L.SpMVPlan(rp, col, v0, n_cols, flags=flags, options=opts) as P, \
            L.SpMVPlan(rp, col, v1, n_cols, flags=flags, options=opts) as F:
        for val in (torch.from_numpy(v1).to(dev), v1):  # device values, host values
            P.set_values(val)
            assert torch.equal(P(xd), F(xd)), (flags, opts, dt)
            if flags == L.PLAN_FORCE_XTILE:
                assert P.layout_digest() == F.layout_digest(), (opts, dt)
            P.set_values(v0)


lengths = [20000] + [3] * 50 + [5000, 4096, 4095, 1, 0, 9000] + [15] * 3000 + [0, 0] + [30000]
rp, col, _ = _csr_from_lengths(lengths, 200_000, 0xDB0, dyadic=True)
for dt in (np.float32, np.float64):
    for opts in ({"xtile_reduce": L.XTILE_REDUCE_PERM}, {"xtile_reduce": L.XTILE_REDUCE_IPERM},
                 {"xtile_part_nnz": 40_000}):
        check(rp, col, 200_000, dt, L.PLAN_FORCE_XTILE, opts)
    for n in (1, 65, 4099):
        lens = rng.integers(1, 9, size=n)
        srp = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(lens, out=srp[1:])
        check(srp, rng.integers(0, n, size=int(srp[-1])).astype(np.int32), n, dt, L.PLAN_FORCE_SELL)
torch.cuda.synchronize()
print("DEBUG SET_VALUES OK")
