"""GPU parity for Y = A·X (lhpc_spmm, libhpc_amd.SpMMPlan) through the C ABI.

The reference per column is the SpMV oracle, S.spmv_oracle(rp, col, val,
X[:, j]), on every row.  Bars are the project's own (tests/test_gpu_spmv.py):
dyadic inputs (dist = 1, values k/8) make every summation order exact, so Y
must equal the rounded oracle bit for bit; U[-1, 1) inputs stay within
|dy| <= 1e-6 * sum|a*x| per row (S.assert_spmv_close), which fp64 accumulation
with one rounding meets on every shape.  Beyond parity: elements j >= k of a
row of Y are never written, and column j of the result is bit-identical for
every k, ldx, ldy and position j (the summation order of an element depends
on its row's structure only), and from run to run.
"""
import functools
import glob
import os
import subprocess

import numpy as np
import pytest

from tests import _support as S

pytestmark = pytest.mark.gpu

GOLDEN_SPMV = sorted(glob.glob(os.path.join(S.GOLDEN, "spmv_*.npz")))
NS = (1, 63, 64, 65, 257, 1000, 4099)
KS = (1, 3, 4, 5, 8, 16, 31, 32, 33, 64, 70)  # panel tails, exact panels, multi-panel with tail
# every n against k in {1, 5, 33} and every k against n in {65, 4099}
EDGE = sorted({(n, k) for n in NS for k in (1, 5, 33)} | {(n, k) for n in (65, 4099) for k in KS})
CANARY = -1234.5


def _dt(lhpc, dtype):
    return lhpc.F32 if dtype == "f32" else lhpc.F64


def _check_block(rp, col, val, X, Y, dyadic):
    """every column of Y against the SpMV oracle on that column of X"""
    assert Y.shape == (rp.shape[0] - 1, X.shape[1]) and Y.dtype == val.dtype
    for j in range(X.shape[1]):
        y64, yr, asum = S.spmv_oracle(rp, col, val, np.ascontiguousarray(X[:, j]))
        if dyadic:
            assert np.array_equal(Y[:, j], yr), f"column {j}: dyadic SpMM must be bit-exact"
        else:
            S.assert_spmv_close(Y[:, j], y64, asum)


def _block(lhpc, dt, dist, rows, k, seed):
    return lhpc.gen_values(dt, dist, rows * k, seed).reshape(rows, k)


def _spmm(lhpc, gpu, rp, col, val, n_cols, X):
    import torch
    with lhpc.SpMMPlan(rp, col, val, n_cols) as plan:
        return plan(torch.from_numpy(X).to(gpu)).cpu().numpy()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n,k", EDGE)
def test_edge_sizes_vs_oracle(lhpc, gpu, n, k, dtype):
    dt = _dt(lhpc, dtype)
    for dist in (0, 1):
        rp, col, val = lhpc.gen_uniform_csr(n, n, min(n, 15), dtype=dt, dist=dist, seed=0xE000 + n)
        X = _block(lhpc, dt, dist, n, k, 0xE100 + n + 7 * k)
        _check_block(rp, col, val, X, _spmm(lhpc, gpu, rp, col, val, n, X), dist == 1)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("k", [1, 5, 32, 33, 70])
def test_leading_dimensions_and_untouched_columns(lhpc, gpu, k, dtype):
    """ldx = k + 3, ldy = k + 5: X a column slice of a wider tensor (no copy),
    Y a column slice of a canary-filled one whose other columns must keep it."""
    import torch
    dt = _dt(lhpc, dtype)
    n, m = 1000, 777
    rp, col, val = lhpc.gen_uniform_csr(n, m, 15, dtype=dt, dist=1, seed=0xE300 + k)
    Xw = _block(lhpc, dt, 1, m, k + 3, 0xE301 + k)
    xw = torch.from_numpy(Xw).to(gpu)
    yw = torch.full((n, k + 5), CANARY, dtype=xw.dtype, device=gpu)
    x, y = xw[:, 2:2 + k], yw[:, 1:1 + k]
    assert (k == 1 or not x.is_contiguous()) and x.stride(0) == k + 3 and y.stride(0) == k + 5
    with lhpc.SpMMPlan(rp, col, val, m) as plan:
        assert plan(x, y) is y
    out = yw.cpu().numpy()
    _check_block(rp, col, val, Xw[:, 2:2 + k], out[:, 1:1 + k], True)
    assert (out[:, 0] == CANARY).all() and (out[:, 1 + k:] == CANARY).all(), "a column >= k of Y was written"


def _long_row_csr(lhpc, dt, dist, seed):
    """rows of exactly 2048 (the last that shares a block), 2049 and 10 000
    nonzeros (a workgroup to themselves) next to rows of 1 and empty rows"""
    lens = np.array([1, 2048, 1, 1, 2049, 0, 1, 10_000, 1, 0, 2048, 2049, 1] + [1] * 300, dtype=np.int64)
    m = 12_000
    rng = np.random.default_rng(seed)
    rp = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(m, size=int(l), replace=False)) for l in lens]).astype(np.int32)
    val = lhpc.gen_values(dt, dist, int(rp[-1]), seed ^ 0x77)
    return rp, col, val, m


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("matrix", ["uniform4099", "longrows"])
def test_column_independence_and_determinism(lhpc, gpu, matrix, dtype):
    """U[-1, 1) values, so a different summation order would show: column j
    of the k = 70 result equals, bit for bit, the k = 1 result on X[:, j],
    column 0 of a k = 5 call on X[:, j:j+5] and the same column under another
    ldx (other panel widths, lanes and strides); two identical calls agree."""
    import torch
    dt = _dt(lhpc, dtype)
    if matrix == "uniform4099":
        n = m = 4099
        rp, col, val = lhpc.gen_uniform_csr(n, n, 15, dtype=dt, dist=0, seed=0xE400)
    else:
        rp, col, val, m = _long_row_csr(lhpc, dt, 0, 0xE401)
        n = rp.shape[0] - 1
    K = 70
    xw = torch.from_numpy(_block(lhpc, dt, 0, m, K + 5, 0xE402)).to(gpu)  # 5 spare columns for the k = 5 windows
    x70 = xw[:, :K]
    with lhpc.SpMMPlan(rp, col, val, m) as plan:
        y70 = plan(x70)
        assert torch.equal(plan(x70), y70), "two identical calls differ"
        y70_ld = plan(x70.contiguous(), torch.empty((n, K + 9), dtype=xw.dtype, device=gpu)[:, 4:4 + K])  # ldx 70, ldy 79
        assert torch.equal(y70_ld, y70), "result depends on ldx / ldy"
        for j in (0, 5, 31, 32, 33, 64, 69):
            assert torch.equal(plan(xw[:, j:j + 1])[:, 0], y70[:, j]), f"column {j}: k = 1 differs from k = 70"
            assert torch.equal(plan(xw[:, j:j + 5])[:, 0], y70[:, j]), f"column {j}: k = 5 differs from k = 70"
            assert torch.equal(plan(xw[:, j:j + 1].contiguous())[:, 0], y70[:, j]), f"column {j}: ldx = 1 differs"
    X = x70.cpu().numpy()
    _check_block(rp, col, val, X[:, [0, 32, 69]], y70.cpu().numpy()[:, [0, 32, 69]], False)


def test_empty_rows_zero_nnz_and_no_rows(lhpc, gpu):
    import torch
    col0, val0 = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32)
    x = torch.ones((7, 5), device=gpu)
    with lhpc.SpMMPlan(np.zeros(11, dtype=np.int32), col0, val0, 7) as plan:
        y = plan(x, torch.full((10, 5), CANARY, device=gpu))
        assert torch.equal(y, torch.zeros((10, 5), device=gpu)), "empty rows must store 0"
        assert plan.info()["nnz"] == 0
    with lhpc.SpMMPlan(np.zeros(1, dtype=np.int32), col0, val0, 7) as plan:
        y = plan(x)
        assert tuple(y.shape) == (0, 5) and plan.info()["n_blocks"] == 0
    # empty rows between full ones
    rp = np.array([0, 0, 3, 3, 3, 5, 5], dtype=np.int32)
    col = np.array([0, 3, 6, 1, 2], dtype=np.int32)
    val = np.array([0.5, -1.25, 2.0, 4.0, -0.125], dtype=np.float32)
    X = _block(lhpc, lhpc.F32, 1, 7, 9, 0xE500)
    _check_block(rp, col, val, X, _spmm(lhpc, gpu, rp, col, val, 7, X), True)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rectangular_and_int64_row_ptr(lhpc, gpu, dtype):
    dt = _dt(lhpc, dtype)
    rp, col, val = lhpc.gen_uniform_csr(1000, 257, 15, dtype=dt, dist=1, seed=0xE600)  # n_cols != n_rows
    X = _block(lhpc, dt, 1, 257, 33, 0xE601)
    _check_block(rp, col, val, X, _spmm(lhpc, gpu, rp, col, val, 257, X), True)
    rp, col, val = lhpc.gen_uniform_csr(257, 1000, 15, dtype=dt, dist=0, seed=0xE602, narrow=False)
    assert rp.dtype == np.int64
    X = _block(lhpc, dt, 0, 1000, 5, 0xE603)
    _check_block(rp, col, val, X, _spmm(lhpc, gpu, rp, col, val, 1000, X), False)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("dist", [0, 1])
def test_block_boundary_and_long_rows(lhpc, gpu, dist, dtype):
    import torch
    dt = _dt(lhpc, dtype)
    rp, col, val, m = _long_row_csr(lhpc, dt, dist, 0xE700 + dist)
    for k in (3, 33):  # panel widths 4, and 32 + 4
        X = _block(lhpc, dt, dist, m, k, 0xE701 + k)
        with lhpc.SpMMPlan(rp, col, val, m) as plan:
            Y = plan(torch.from_numpy(X).to(gpu)).cpu().numpy()
            assert plan.info()["n_long_rows"] == 3  # 2049, 10 000, 2049
        _check_block(rp, col, val, X, Y, dist == 1)


@functools.lru_cache(maxsize=None)
def _powerlaw(dtype_code):
    import libhpc_amd as L
    return L.gen_powerlaw_csr(20_000, 20_000, lmax=10_000, dtype=dtype_code, seed=0xE800)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("k", [8, 32])
def test_powerlaw_vs_oracle(lhpc, gpu, k, dtype):
    dt = _dt(lhpc, dtype)
    rp, col, val = _powerlaw(dt)
    X = _block(lhpc, dt, 0, 20_000, k, 0xE801 + k)
    _check_block(rp, col, val, X, _spmm(lhpc, gpu, rp, col, val, 20_000, X), False)


def test_64bit_element_offsets(lhpc, gpu):
    """(n_cols - 1)·ldx >= 2^31: X is a 4-column slice of a 70 000 × 32 768
    fp32 tensor (9.2 GB, only the slice is initialised) and every row reads
    its last row.  Dyadic, bit-exact."""
    import torch
    n, m, k, ldx = 1000, 70_000, 4, 32_768
    assert (m - 1) * ldx >= 2 ** 31
    rp, col, val = lhpc.gen_uniform_csr(n, m, 4, dtype=lhpc.F32, dist=1, seed=0xE900)
    col[3::4] = m - 1  # the largest column of every (sorted, distinct) row
    X = _block(lhpc, lhpc.F32, 1, m, k, 0xE901)
    big = torch.empty((m, ldx), dtype=torch.float32, device=gpu)
    x = big[:, :k]
    x.copy_(torch.from_numpy(X))
    assert x.stride(0) == ldx
    with lhpc.SpMMPlan(rp, col, val, m) as plan:
        Y = plan(x).cpu().numpy()
    del big, x
    _check_block(rp, col, val, X, Y, True)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_host_buffers_and_device_plan_match(lhpc, gpu, dtype):
    """host numpy buffers (packed and strided) equal device buffers bit for
    bit; a plan from device tensors (PLAN_DEVICE_INPUT) equals the host-built one"""
    import torch
    dt = _dt(lhpc, dtype)
    n, m, k = 4099, 3001, 37
    rp, col, val = lhpc.gen_uniform_csr(n, m, 15, dtype=dt, dist=0, seed=0xEA00)
    Xw = _block(lhpc, dt, 0, m, k + 3, 0xEA01)
    X = Xw[:, 1:1 + k]
    with lhpc.SpMMPlan(rp, col, val, m) as plan:
        yd = plan(torch.from_numpy(Xw).to(gpu)[:, 1:1 + k]).cpu().numpy()
        assert np.array_equal(plan(np.ascontiguousarray(X)), yd)
        Yw = np.full((n, k + 5), CANARY, dtype=val.dtype)
        assert np.array_equal(plan(X, Yw[:, 2:2 + k]), yd)  # ldx = k + 3, ldy = k + 5: strided 2-D copies
        assert (Yw[:, :2] == CANARY).all() and (Yw[:, 2 + k:] == CANARY).all()
        assert np.array_equal(plan(np.ascontiguousarray(X[:, :3])), yd[:, :3])  # the stage is reused for a smaller k
        host_info = plan.info()
    t = [torch.from_numpy(a).to(gpu) for a in (rp, col, val)]
    with lhpc.SpMMPlan(*t, m) as plan:
        assert np.array_equal(plan(torch.from_numpy(Xw).to(gpu)[:, 1:1 + k]).cpu().numpy(), yd)
        dev_info = plan.info()
    for key in ("dtype", "n_rows", "n_cols", "nnz", "n_blocks", "n_long_rows", "panel_max"):
        assert host_info[key] == dev_info[key], key
    assert host_info["panel_max"] == 32 and host_info["n_blocks"] > 1
    _check_block(rp, col, val, X[:, [0, 36]], yd[:, [0, 36]], False)


def test_validate_rejects_bad_column_host_and_device(lhpc, gpu):
    import torch
    rp, col, val = lhpc.gen_uniform_csr(65, 65, 15, dtype=lhpc.F32, seed=0xEB00)
    bad = col.copy()
    bad[100] = 65  # == n_cols
    for flags in (0, lhpc.PLAN_VALIDATE):
        with pytest.raises(lhpc.LhpcError) as e:
            lhpc.SpMMPlan(rp, bad, val, 65, flags=flags)
        assert e.value.status == -2
        with pytest.raises(lhpc.LhpcError) as e:
            lhpc.SpMMPlan(*(torch.from_numpy(a).to(gpu) for a in (rp, bad, val)), 65, flags=flags)
        assert e.value.status == -2
    with pytest.raises(lhpc.LhpcError) as e:  # a kernel family cannot be forced
        lhpc.SpMMPlan(rp, col, val, 65, flags=lhpc.PLAN_FORCE_ADAPTIVE)
    assert e.value.status == -1


def test_call_argument_errors(lhpc, gpu):
    import torch
    rp, col, val = lhpc.gen_uniform_csr(65, 65, 15, dtype=lhpc.F32, seed=0xEC00)
    x = torch.ones((65, 8), device=gpu)
    y = torch.full((65, 8), CANARY, device=gpu)
    with lhpc.SpMMPlan(rp, col, val, 65) as plan:
        call = lambda k, X, ldx, Y, ldy: lhpc.lib.lhpc_spmm(plan._h, k, X, ldx, Y, ldy, 1, None)  # noqa: E731
        assert call(0, x.data_ptr(), 8, y.data_ptr(), 8) == -1
        assert call(8, x.data_ptr(), 7, y.data_ptr(), 8) == -1
        assert call(8, x.data_ptr(), 8, y.data_ptr(), 7) == -1
        assert call(8, None, 8, y.data_ptr(), 8) == -1
        assert call(8, x.data_ptr(), 8, None, 8) == -1
        assert lhpc.lib.lhpc_spmm_plan_info_get(plan._h, None) == -1
        torch.cuda.synchronize()
        assert (y == CANARY).all()
        with pytest.raises(ValueError):
            plan(x[:, ::2])  # non-unit inner stride
        with pytest.raises(ValueError):
            plan(x[:64])  # too few rows
        with pytest.raises(ValueError):
            plan(x, y[:, :4])  # Y narrower than X
        with pytest.raises(TypeError):
            plan(x.double())
        with pytest.raises(ValueError):
            plan(x, np.empty((65, 8), dtype=np.float32))  # device X, host Y


@pytest.mark.parametrize("path", GOLDEN_SPMV, ids=lambda p: os.path.basename(p)[5:-4])
def test_golden(lhpc, gpu, path):
    """every SpMV fixture with X[:, j] = its x rolled by j (k = 5): column 0
    against the exact-arithmetic y as tests/test_gpu_spmv.py::test_golden
    does, the other columns against the oracle"""
    g = S.load_golden(os.path.basename(path))
    rp, col, val, x = g["row_ptr"], g["col_idx"], g["val"], g["x"]
    X = np.stack([np.roll(x, j) for j in range(5)], axis=1)
    Y = _spmm(lhpc, gpu, rp, col, val, int(g["n_cols"]), X)
    dyadic = "dyadic" in path
    if dyadic:
        assert np.array_equal(Y[:, 0], g["y_exact"].astype(val.dtype)), "dyadic SpMM must be bit-exact"
    else:
        _, _, asum = S.spmv_oracle(rp, col, val, x)
        S.assert_spmv_close(Y[:, 0], g["y_exact"], asum)
    _check_block(rp, col, val, X[:, 1:], Y[:, 1:], dyadic)


def test_cpp_drop_in(gpu, tmp_path):
    """sparse::SpMMPlan / sparse::spmm (include/sparse/SpMM.hpp) on 2-D flat
    arrays with ghost cells and on raw HBM pointers: tests/cpp/test_spmm_api.cpp,
    built here with one compiler command against include/ and libhpc_amd/_lib."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    libdir = os.path.join(S.ROOT, "libhpc_amd", "_lib")
    exe = str(tmp_path / "test_spmm_api")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                    "-I" + os.path.join(S.ROOT, "include"), "-I" + os.path.join(S.ROOT, "include", "hpc"),
                    "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    os.path.join(S.ROOT, "tests", "cpp", "test_spmm_api.cpp"), "-o", exe,
                    "-L" + libdir, "-llhpc", "-Wl,-rpath," + libdir,
                    "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "spmm cpp api: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ------------------------------------------------------------------ non-finite X
_NAN_CASES = {}


def _nan_case(lhpc, matrix, dt):
    """(row_ptr, col_idx, val, n_cols, poisoned columns): dyadic values; the
    poisoned columns of x — the first, the last, 63 / 64 and an interior one —
    have entries planted in chosen rows (rows of 1, of 15, the 2048-, a 2049-
    and the 10 000-entry row), so nothing is left to chance."""
    if (matrix, dt) not in _NAN_CASES:
        if matrix == "uniform4099":
            m = 4099
            rp, col, val = lhpc.gen_uniform_csr(m, m, 15, dtype=dt, dist=1, seed=0xED00)
            targets = [(10, 2000), (12, 2002), (14, 2004), (16, 2006), (18, 2008)]
        else:
            rp, col, val, m = _long_row_csr(lhpc, dt, 1, 0xED01)
            targets = [(0, 1, 20), (1, 22), (4, 24), (7, 26), (7, 10, 28)]  # row 1: 2048, 4: 2049, 7: 10 000 entries
        col = col.copy()
        poison = [0, m - 1, 63, 64, (m // 2) | 1]
        for k, (c, rows) in enumerate(zip(poison, targets)):
            for r in rows:
                S.plant_column(rp, col, r, c, "first" if k % 2 == 0 else "last", protect=poison)
        for r in range(rp.size - 1):
            assert (np.diff(col[rp[r]:rp[r + 1]]) > 0).all()
        _NAN_CASES[(matrix, dt)] = (rp, col, val, m, np.array(poison))
    return _NAN_CASES[(matrix, dt)]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("k,j0", [(5, 0), (5, 4), (33, 0), (33, 31), (33, 32)])
@pytest.mark.parametrize("matrix", ["uniform4099", "longrows"])
def test_nan_in_one_column_of_x_stays_there(lhpc, gpu, matrix, k, j0, dtype):
    """NaN in X[c, j0] for a few columns c of A, in one column j0 of the block
    only (the first and the last of a panel, and of the 1-wide tail panel of
    k = 33): every other column of Y keeps the clean call's bits (clean: those
    entries 0.5; checked against the oracle), column j0 is NaN exactly in the
    rows whose fp64 row sum is (tests/_support.py assert_nonfinite_stays).
    lhpc_spmm_dot on the same inputs stores the same Y, and its dots[j] for
    j != j0 keep the clean call's bits while dots[j0] is NaN.  A panel-tail
    lane or a padded product that read another column's x would show."""
    import torch
    dt = _dt(lhpc, dtype)
    rp, col, val, m, poison = _nan_case(lhpc, matrix, dt)
    n = rp.shape[0] - 1
    Xc = _block(lhpc, dt, 1, m, k, 0xED10 + k)
    Xc[poison, j0] = 0.5
    Xb = Xc.copy()
    Xb[poison, j0] = np.nan
    W = _block(lhpc, dt, 1, n, k, 0xED20 + k)
    e = S.row_sums_fp64(rp, col, val, np.ascontiguousarray(Xb[:, j0]))
    with lhpc.SpMMPlan(rp, col, val, m) as plan:
        xc, xb, w = (torch.from_numpy(a).to(gpu) for a in (Xc, Xb, W))
        nan_y = lambda: torch.full((n, k), float("nan"), dtype=xc.dtype, device=gpu)  # noqa: E731
        Yb = plan(xb, nan_y()).cpu().numpy()
        Yc = plan(xc, nan_y()).cpu().numpy()  # after the poisoned call, on the same plan
        Ydb, dots_b = lhpc.spmm_dot(plan, xb, w, nan_y())
        Ydc, dots_c = lhpc.spmm_dot(plan, xc, w, nan_y())
        Ydb, Ydc, dots_b, dots_c = (t.cpu().numpy() for t in (Ydb, Ydc, dots_b, dots_c))
    cols = sorted({0, j0, k - 1})
    _check_block(rp, col, val, Xc[:, cols], Yc[:, cols], True)
    others = [j for j in range(k) if j != j0]
    assert np.array_equal(Yb[:, others], Yc[:, others]), "NaN in one column of X changed another column of Y"
    aff = S.assert_nonfinite_stays(Yb[:, j0], Yc[:, j0], e)
    assert aff.sum() >= 5 and aff.mean() <= 0.10 and S.touches_unaffected_neighbour(aff)
    assert np.array_equal(Ydb, Yb, equal_nan=True) and np.array_equal(Ydc, Yc)
    assert np.array_equal(dots_b[others], dots_c[others]) and np.isnan(dots_b[j0])
    assert np.isfinite(dots_c).all()
