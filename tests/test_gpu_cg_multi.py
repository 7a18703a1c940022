"""GPU checks of lhpc_spmm_dot and lhpc_cg_solve_multi (libhpc_amd.spmm_dot /
cg_multi): k conjugate-gradient recurrences in step on one SpMM plan.

Bars are the project's own.  spmm_dot: Y bit-identical to SpMMPlan.__call__,
dots within 1e-12·Σ|W·Y| of numpy's fp64 dot of the stored Y
(test_gpu_cg.py::test_cg_building_blocks).  Solver, per column against
S.cg_oracle: fp64 — iteration count ±1, residual ≤ tol, ‖x − x_o‖ ≤ 1e-8·‖x_o‖
at tol 1e-10 (test_cg_fp64_matches_oracle); fp32 — within 1e-4 of the fp64
solution at tol 1e-5 (test_cg_fp32).  Beyond parity, the property the design
rests on: column j of a k-column call goes through exactly the operations of
the one-column call on that column, so dots[j], X_j, iters[j] and resid[j]
are bit-identical for every k, leading dimension and position j, and from
run to run — which is what catches indexing, stride, panel and freeze-mask
bugs.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _support as S

pytestmark = pytest.mark.gpu

CANARY = -1234.5
COLS = (0, 5, 31, 32, 33, 64, 69)


def _dt(lhpc, dtype):
    return lhpc.F32 if dtype == "f32" else lhpc.F64


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(gpu)  # a copy: the shared inputs are read-only


def _block(lhpc, dt, rows, k, seed):
    return lhpc.gen_values(dt, 0, rows * k, seed).reshape(rows, k)  # U[-1, 1)


def _long_row_csr(lhpc, dt, seed):
    """tests/test_gpu_spmm.py's long-row matrix: rows of exactly 2048 (the last
    that shares a block), 2049 and 10 000 nonzeros (a workgroup to themselves)
    next to rows of 1 and empty rows"""
    lens = np.array([1, 2048, 1, 1, 2049, 0, 1, 10_000, 1, 0, 2048, 2049, 1] + [1] * 300, dtype=np.int64)
    m = 12_000
    rng = np.random.default_rng(seed)
    rp = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(m, size=int(l), replace=False)) for l in lens]).astype(np.int32)
    val = lhpc.gen_values(dt, 0, int(rp[-1]), seed ^ 0x77)
    return rp, col, val, m


# ------------------------------------------------------------------ spmm_dot
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("matrix", ["uniform4099", "longrows"])
def test_spmm_dot_parity_and_column_identity(lhpc, gpu, matrix, dtype):
    import torch
    dt = _dt(lhpc, dtype)
    if matrix == "uniform4099":
        n = m = 4099
        rp, col, val = lhpc.gen_uniform_csr(n, n, 15, dtype=dt, dist=0, seed=0xF400)
    else:
        rp, col, val, m = _long_row_csr(lhpc, dt, 0xF401)
        n = rp.shape[0] - 1
    K = 70
    xw = _dev(gpu, _block(lhpc, dt, m, K + 5, 0xF402))  # 5 spare columns for the k = 5 windows
    ww = _dev(gpu, _block(lhpc, dt, n, K + 5, 0xF403))  # W != X
    x70, w70 = xw[:, :K], ww[:, :K]
    with lhpc.SpMMPlan(rp, col, val, m) as plan:
        want_y = plan(x70)
        yw = torch.full((n, K + 4), CANARY, dtype=xw.dtype, device=gpu)
        y70, d70 = lhpc.spmm_dot(plan, x70, w70, Y=yw[:, 1:1 + K])
        assert torch.equal(y70, want_y), "Y differs from lhpc_spmm's"
        assert (yw[:, 0] == CANARY).all() and (yw[:, 1 + K:] == CANARY).all(), "a column >= k of Y was written"
        prod = w70.cpu().numpy().astype(np.float64) * y70.cpu().numpy().astype(np.float64)
        got = d70.cpu().numpy()
        bar = 1e-12 * np.abs(prod).sum(axis=0)
        err = np.abs(got - prod.sum(axis=0))
        print(f"spmm_dot {matrix} {dtype}: max err / bar = {(err / bar).max():.3g}")
        assert (err <= bar).all(), (err / bar).max()
        y2, d2 = lhpc.spmm_dot(plan, x70, w70)
        assert torch.equal(d2, d70) and torch.equal(y2, want_y), "two identical calls differ"
        # other leading dimensions: ldx = ldw = 70 (packed), ldy = 79
        _, d_ld = lhpc.spmm_dot(plan, x70.contiguous(), w70.contiguous(),
                                Y=torch.empty((n, K + 9), dtype=xw.dtype, device=gpu)[:, 4:4 + K])
        assert torch.equal(d_ld, d70), "dots depend on ldx / ldy / ldw"
        for j in COLS:
            y1, d1 = lhpc.spmm_dot(plan, xw[:, j:j + 1], ww[:, j:j + 1])
            assert d1[0] == d70[j] and torch.equal(y1[:, 0], want_y[:, j]), f"column {j}: k = 1 differs from k = 70"
            _, d5 = lhpc.spmm_dot(plan, xw[:, j:j + 5], ww[:, j:j + 5])
            assert d5[0] == d70[j], f"column {j}: k = 5 window differs from k = 70"
            _, d1c = lhpc.spmm_dot(plan, xw[:, j:j + 1].contiguous(), ww[:, j:j + 1].contiguous())
            assert d1c[0] == d70[j], f"column {j}: ld = 1 differs"


def test_spmm_dot_square_w_is_x_and_empty_matrices(lhpc, gpu):
    import torch
    rp, col, val = S.laplacian_2d(64, 48)
    n = rp.size - 1
    x = _dev(gpu, _block(lhpc, lhpc.F64, n, 5, 0xF410))
    with lhpc.SpMMPlan(rp, col, val, n) as plan:
        y, d = lhpc.spmm_dot(plan, x, x)  # the CG use, p·Ap
        prod = (x * y).cpu().numpy()
        assert (np.abs(d.cpu().numpy() - prod.sum(axis=0)) <= 1e-12 * np.abs(prod).sum(axis=0)).all()
    col0, val0 = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32)
    x = torch.ones((7, 5), device=gpu)
    with lhpc.SpMMPlan(np.zeros(11, dtype=np.int32), col0, val0, 7) as plan:  # all rows empty
        w = torch.ones((10, 5), device=gpu)
        y, d = lhpc.spmm_dot(plan, x, w, Y=torch.full((10, 5), CANARY, device=gpu),
                             out=torch.full((5,), CANARY, dtype=torch.float64, device=gpu))
        assert torch.equal(y, torch.zeros((10, 5), device=gpu)) and (d == 0).all()
    with lhpc.SpMMPlan(np.zeros(1, dtype=np.int32), col0, val0, 7) as plan:  # no rows
        # one spare row: an empty tensor has no pointer, and a null W or Y is an argument error
        y, d = lhpc.spmm_dot(plan, x, torch.ones((1, 5), device=gpu), Y=torch.full((1, 5), CANARY, device=gpu),
                             out=torch.full((5,), CANARY, dtype=torch.float64, device=gpu))
        assert (d == 0).all() and (y == CANARY).all()


# -------------------------------------------------------------------- solver
@functools.lru_cache(maxsize=None)
def _oracle_block(shape, k, shift=0.0, tol=1e-10):
    """(rp, col, val, B, per-column oracle results) — computed once, shared, never modified"""
    rp, col, val = S.laplacian_2d(*shape, shift=shift)
    n = rp.size - 1
    B = np.random.default_rng(n + k).uniform(-1, 1, (n, k))
    ref = [S.cg_oracle(rp, col, val, np.ascontiguousarray(B[:, j]), tol=tol, max_iter=5000) for j in range(k)]
    for a in (rp, col, val, B):
        a.setflags(write=False)
    return rp, col, val, B, ref


@pytest.mark.parametrize("shape,k", [((64, 48), 5), ((200, 150), 5), ((7, 1), 5), ((64, 48), 33), ((64, 48), 70)])
def test_cg_multi_fp64_matches_oracle(lhpc, gpu, shape, k):
    rp, col, val, B, ref = _oracle_block(shape, k)
    n = rp.size - 1
    with lhpc.SpMMPlan(rp, col, val, n) as plan:
        X, iters, resid = lhpc.cg_multi(plan, _dev(gpu, B), tol=1e-10, max_iter=5000)
    X = X.cpu().numpy()
    assert iters.dtype == np.int32 and resid.dtype == np.float64 and iters.shape == resid.shape == (k,)
    for j, (want, it_o, _) in enumerate(ref):
        assert abs(int(iters[j]) - it_o) <= 1 and resid[j] <= 1e-10, (j, iters[j], it_o, resid[j])
        assert np.linalg.norm(X[:, j] - want) <= 1e-8 * np.linalg.norm(want), j


def test_cg_multi_fp32(lhpc, gpu):
    rp, col, val = S.laplacian_2d(128, 128, dtype=np.float32, shift=0.5)
    n, k = rp.size - 1, 5
    B = np.random.default_rng(3).uniform(-1, 1, (n, k)).astype(np.float32)
    with lhpc.SpMMPlan(rp, col, val, n) as plan:
        X, iters, resid = lhpc.cg_multi(plan, _dev(gpu, B), tol=1e-5, max_iter=5000, check_every=5)
    X = X.cpu().numpy().astype(np.float64)
    assert (iters % 5 == 0).all() and (iters > 0).all() and (resid <= 1e-5).all()
    for j in range(k):
        want, _, _ = S.cg_oracle(rp, col, val, B[:, j].astype(np.float64), tol=1e-12, max_iter=5000)
        assert np.linalg.norm(X[:, j] - want) <= 1e-4 * np.linalg.norm(want), j


NX, NY = 64, 48


@functools.lru_cache(maxsize=None)
def _staggered():
    """(64, 48) Laplacian with shift 0.5 and six right-hand sides that stop at
    different checks: 0, the lowest eigenvector (one iteration), the same
    scaled by 1e6, three random ones (S.cg_oracle: 0, 1, 1, 46, 46, 46
    iterations at tol 1e-10)."""
    rp, col, val = S.laplacian_2d(NX, NY, shift=0.5)
    n = rp.size - 1
    ev = np.outer(np.sin(np.pi * (np.arange(NY) + 1) / (NY + 1)), np.sin(np.pi * (np.arange(NX) + 1) / (NX + 1))).ravel()
    B = np.zeros((n, 6))
    B[:, 1] = ev
    B[:, 2] = 1e6 * ev
    B[:, 3:] = np.random.default_rng(0xC6).uniform(-1, 1, (n, 3))
    for a in (rp, col, val, B):
        a.setflags(write=False)
    return rp, col, val, B


KW = dict(tol=1e-10, max_iter=5000, check_every=3)


@pytest.fixture(scope="module")
def staggered(lhpc, gpu):
    """the matrix, B, and the k = 1 solve of every column on its own: (x, iters, resid)"""
    rp, col, val, B = _staggered()
    n = rp.size - 1
    singles = []
    with lhpc.SpMMPlan(rp, col, val, n) as plan:
        for j in range(6):
            x, it, res = lhpc.cg_multi(plan, _dev(gpu, B[:, j:j + 1]), **KW)
            singles.append((x[:, 0].clone(), int(it[0]), float(res[0])))
    return rp, col, val, B, singles


def _same_as_single(X, iters, resid, pos, singles):
    import torch
    for c, j in enumerate(pos):
        x1, it1, res1 = singles[c]
        assert int(iters[j]) == it1, (c, j, iters[j], it1)
        assert resid[j] == res1 or (np.isnan(resid[j]) and np.isnan(res1)), (c, j, resid[j], res1)
        assert torch.equal(X[:, j], x1), f"column {c} at position {j}: X differs from its k = 1 solve"


def test_columns_stop_at_different_times(lhpc, gpu, staggered):
    import torch
    rp, col, val, B, singles = staggered
    n = rp.size - 1
    its = [s[1] for s in singles]
    print("k = 1 iterations:", its)
    assert its[0] == 0 and len(set(its)) > 1 and all(i % 3 == 0 for i in its)
    with lhpc.SpMMPlan(rp, col, val, n) as plan:
        X, iters, resid = lhpc.cg_multi(plan, _dev(gpu, B), **KW)
        _same_as_single(X, iters, resid, range(6), singles)
        assert iters[0] == 0 and resid[0] == 0.0 and torch.count_nonzero(X[:, 0]) == 0
        X2, iters2, resid2 = lhpc.cg_multi(plan, _dev(gpu, B), **KW)  # run to run
        assert torch.equal(X2, X) and (iters2 == iters).all() and (resid2 == resid).all()


def test_columns_are_position_independent_at_k33(lhpc, gpu, staggered):
    """the six columns at positions 0, 5, 17, 24, 31 and 32 (both sides of the
    32-column panel edge) of a 33-column block, random filler elsewhere"""
    rp, col, val, B, singles = staggered
    n = rp.size - 1
    pos = (0, 5, 17, 24, 31, 32)
    B33 = np.random.default_rng(0xC7).uniform(-1, 1, (n, 33))
    B33[:, pos] = B
    with lhpc.SpMMPlan(rp, col, val, n) as plan:
        X, iters, resid = lhpc.cg_multi(plan, _dev(gpu, B33), **KW)
    _same_as_single(X, iters, resid, pos, singles)
    assert (resid <= 1e-10).all()


def test_column_slices_of_wider_tensors(lhpc, gpu, staggered):
    import torch
    rp, col, val, B, singles = staggered
    n = rp.size - 1
    bw = torch.full((n, 6 + 3), CANARY, dtype=torch.float64, device=gpu)
    xw = torch.full((n, 6 + 5), CANARY, dtype=torch.float64, device=gpu)
    b, x = bw[:, 2:8], xw[:, 1:7]
    b.copy_(_dev(gpu, B))
    x.zero_()
    keep = bw.clone()
    assert b.stride(0) == 9 and x.stride(0) == 11
    with lhpc.SpMMPlan(rp, col, val, n) as plan:
        X, iters, resid = lhpc.cg_multi(plan, b, X=x, **KW)
    assert X is x
    _same_as_single(x, iters, resid, range(6), singles)
    assert torch.equal(bw, keep), "B (or a canary beside it) was written"
    assert (xw[:, 0] == CANARY).all() and (xw[:, 7:] == CANARY).all(), "a column >= k of X was written"


def test_warm_start_max_iter_and_device_bytes(lhpc, gpu):
    import torch
    rp, col, val, B, ref = _oracle_block((64, 48), 5)
    n, k = rp.size - 1, 5
    b = _dev(gpu, B)
    with lhpc.SpMMPlan(rp, col, val, n) as plan:
        before = plan.info()["device_bytes"]
        x1, it1, _ = lhpc.cg_multi(plan, b, tol=1e-12, max_iter=5000)
        assert plan.info()["device_bytes"] - before >= 3 * n * k * 8
        x2, it2, _ = lhpc.cg_multi(plan, b, X=x1.clone(), tol=1e-10, max_iter=5000)  # warm start
        assert (it2 <= 1).all() and torch.allclose(x2, x1, rtol=0, atol=1e-11)
        _, it3, res3 = lhpc.cg_multi(plan, b, tol=1e-10, max_iter=7, check_every=4)  # cut short
        assert (it3 == 7).all() and (res3 > 1e-10).all()
        x0 = torch.zeros((n, k), dtype=torch.float64, device=gpu)
        _, it0, res0 = lhpc.cg_multi(plan, b, X=x0, tol=1e-10, max_iter=0)
        assert (it0 == 0).all() and torch.count_nonzero(x0) == 0 and np.allclose(res0, 1.0, rtol=1e-12, atol=0)
        grown = plan.info()["device_bytes"]
        lhpc.cg_multi(plan, b[:, :2], tol=1e-10)  # a narrower solve reuses the work
        assert plan.info()["device_bytes"] == grown
        plan.close()
        plan.close()


def test_breakdown_is_reported_and_the_other_column_is_solved(lhpc, gpu):
    """A = [[0,1],[1,0]] ⊕ I₂, B = [e0, e2]: p·Ap = 0 on column 0's first step
    (non-finite residual, LHPC_ERR_INTERNAL); column 1 converges in one."""
    import torch
    rp = np.array([0, 1, 2, 3, 4], np.int32)
    col = np.array([1, 0, 2, 3], np.int32)
    val = np.ones(4)
    B = np.zeros((4, 2))
    B[0, 0] = B[2, 1] = 1.0
    b = _dev(gpu, B)
    x = torch.zeros((4, 2), dtype=torch.float64, device=gpu)
    iters = np.full(2, -1, np.int32)
    resid = np.full(2, CANARY)
    with lhpc.SpMMPlan(rp, col, val, 4) as plan:
        st = lhpc.lib.lhpc_cg_solve_multi(plan._h, 2, b.data_ptr(), 2, x.data_ptr(), 2, 1e-10, 50, 1,
                                          iters.ctypes.data, resid.ctypes.data, None)
        assert st == -6 and not np.isfinite(resid[0]) and iters[0] == 1
        assert iters[1] == 1 and resid[1] <= 1e-10
        assert np.array_equal(x.cpu().numpy()[:, 1], B[:, 1])
        with pytest.raises(lhpc.LhpcError) as e:
            lhpc.cg_multi(plan, b, tol=1e-10, max_iter=50)
        assert e.value.status == -6 and not np.isfinite(e.value.resid[0]) and e.value.iters[1] == 1
        xs, its, res = lhpc.cg_multi(plan, b[:, 1:2], tol=1e-10, max_iter=50)  # the plan is free again
        assert its[0] == 1 and res[0] <= 1e-10 and np.array_equal(xs.cpu().numpy()[:, 0], B[:, 1])


def test_non_square_plan_is_an_argument_error(lhpc, gpu):
    import torch
    rp, col, val = lhpc.gen_uniform_csr(65, 70, 5, dtype=lhpc.F32, seed=0xF500)
    b = torch.ones((70, 2), device=gpu)
    x = torch.zeros((70, 2), device=gpu)
    with lhpc.SpMMPlan(rp, col, val, 70) as plan:
        assert lhpc.lib.lhpc_cg_solve_multi(plan._h, 2, b.data_ptr(), 2, x.data_ptr(), 2, 1e-8, 10, 1, None, None,
                                            None) == -1
        with pytest.raises(lhpc.LhpcError) as e:
            lhpc.cg_multi(plan, b, X=x)
        assert e.value.status == -1
    assert torch.count_nonzero(x) == 0


def test_cpp_drop_in(gpu, tmp_path):
    """sparse::cg and sparse::spmm_dot (include/sparse/SpMM.hpp):
    tests/cpp/test_cg_multi_api.cpp, built here with one compiler command
    against include/ and libhpc_amd/_lib."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.join(S.ROOT, "libhpc_amd", "_lib")
    exe = str(tmp_path / "test_cg_multi_api")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                    "-I" + os.path.join(S.ROOT, "include"), "-I" + os.path.join(S.ROOT, "include", "hpc"),
                    "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    os.path.join(S.ROOT, "tests", "cpp", "test_cg_multi_api.cpp"), "-o", exe,
                    "-L" + libdir, "-llhpc", "-Wl,-rpath," + libdir,
                    "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cg multi cpp api: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def test_debug_build_runs_trap_free(gpu):
    """The bounds-trap, synchronous-check build of the same ABI runs the new
    kernels on valid inputs without a trap (tests/debug_build_check_cg_multi.py,
    a process of its own: it loads another library)."""
    so = os.path.join(S.ROOT, "libhpc_amd", "_lib_debug", "liblhpc.so")
    r = subprocess.run([sys.executable, os.path.join(S.ROOT, "tests", "debug_build_check_cg_multi.py")],
                       env=dict(os.environ, LHPC_LIB_PATH=so), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "DEBUG BUILD OK (cg_multi)" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
