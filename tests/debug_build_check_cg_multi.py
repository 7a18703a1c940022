"""Run by tests/test_gpu_cg_multi.py with LHPC_LIB_PATH naming the debug build
(-DLHPC_DEBUG_BOUNDS -DLHPC_DEBUG_SYNC): lhpc_spmm_dot and lhpc_cg_solve_multi
on valid inputs — odd sizes, long rows, a panel tail, leading dimensions —
must run without a bounds trap and give the product build's answers (the
debug flags change no arithmetic).  Valid inputs only: a trap is a GPU fault,
so nothing here provokes one."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import libhpc_amd as L  # noqa: E402
from tests import _support as S  # noqa: E402

assert L.lib.lhpc_build_flags() & 2, "not the debug build"
dev = torch.device("cuda:0")

# spmm_dot: rows of 1, 2048, 2049, 10 000 and 0 nonzeros, k = 33 (a full panel and a tail of one)
lens = np.array([1, 2048, 1, 2049, 0, 10_000, 1, 0] + [1] * 300, dtype=np.int64)
m, k = 12_000, 33
rng = np.random.default_rng(0xDB6)
rp = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
col = np.concatenate([np.sort(rng.choice(m, size=int(l), replace=False)) for l in lens]).astype(np.int32)
val = rng.uniform(-1, 1, int(rp[-1]))
n = rp.size - 1
xw = torch.from_numpy(rng.uniform(-1, 1, (m, k + 3))).to(dev)
ww = torch.from_numpy(rng.uniform(-1, 1, (n, k + 2))).to(dev)
with L.SpMMPlan(rp, col, val, m) as plan:
    y, d = L.spmm_dot(plan, xw[:, 1:1 + k], ww[:, :k])
    assert torch.equal(y, plan(xw[:, 1:1 + k]))
    prod = (ww[:, :k] * y).cpu().numpy()
    assert (np.abs(d.cpu().numpy() - prod.sum(axis=0)) <= 1e-12 * np.abs(prod).sum(axis=0)).all()

# cg_multi: n = 3071 (a partial last row tile), k = 33, B and X slices of wider tensors, columns that stop apart
rp, col, val = S.laplacian_2d(83, 37, shift=0.5)
n = rp.size - 1
B = rng.uniform(-1, 1, (n, k))
B[:, 0] = 0.0
bw = torch.zeros((n, k + 2), dtype=torch.float64, device=dev)
bw[:, 2:] = torch.from_numpy(B).to(dev)
xw = torch.zeros((n, k + 1), dtype=torch.float64, device=dev)
with L.SpMMPlan(rp, col, val, n) as plan:
    X, iters, resid = L.cg_multi(plan, bw[:, 2:], X=xw[:, :k], tol=1e-10, max_iter=2000, check_every=3)
assert iters[0] == 0 and (iters[1:] > 0).all() and (resid <= 1e-10).all(), (iters, resid)
want, _, _ = S.cg_oracle(rp, col, val, np.ascontiguousarray(B[:, k - 1]), tol=1e-12, max_iter=5000)
assert np.linalg.norm(X[:, k - 1].cpu().numpy() - want) <= 1e-8 * np.linalg.norm(want)
assert torch.count_nonzero(xw[:, k]) == 0
torch.cuda.synchronize()
print("DEBUG BUILD OK (cg_multi)")
