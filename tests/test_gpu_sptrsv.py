"""lhpc_sptrsv on the GPU: the level-scheduled triangular solve against the
oracle of tests/test_sptrsv_api.py, bit for bit (integer views), on every test
matrix × {fp32, fp64} × {lower, upper} × {unit, non-unit} × chain_rows
∈ {−1, 0, 64, 2048}; the same bits through host buffers, device buffers, a
non-null stream, x aliasing b, a LHPC_PLAN_DEVICE_INPUT plan and a captured
graph; the plan info; set_values; non-finite right-hand sides and a zero
diagonal; a Gauss–Seidel iteration; the C++ surface; the debug build."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _support as S
from tests.test_sptrsv_api import (MATRICES, build_cpp, gauss_seidel_oracle, gauss_seidel_problem, levels_oracle,
                                   matrix, rhs, solution, sptrsv_oracle)

pytestmark = pytest.mark.gpu

CHAIN_ROWS = (-1, 0, 64, 2048)
DTYPES = [np.float32, np.float64]
IDS = dict(ids=lambda v: getattr(v, "__name__", None))


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def dev(gpu, a):
    import torch
    return torch.from_numpy(np.array(a)).to(gpu)


# ------------------------------------------------------------------ bit equality with the oracle
@pytest.mark.parametrize("unit", [False, True], ids=["nonunit", "unit"])
@pytest.mark.parametrize("upper", [False, True], ids=["lower", "upper"])
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("name", MATRICES)
def test_bits_equal_the_oracle(lhpc, gpu, name, dtype, upper, unit):
    """Every chain_rows gives the oracle's bits: −1 one launch per level, 0
    the automatic threshold, 64 grid steps for grid_rb / mixed's big levels,
    2048 grid_rb's 1056-row levels (17 slices) inside the chain workgroup,
    whose 16 waves wrap over them."""
    rp, col, val = matrix(name, upper, dtype, unit)
    n = rp.size - 1
    want = solution(name, upper, dtype, unit)
    bd = dev(gpu, rhs(n, dtype))
    for chain_rows in CHAIN_ROWS:
        with lhpc.SpTRSVPlan(rp, col, val, upper=upper, unit_diag=unit, chain_rows=chain_rows) as plan:
            x = plan(bd)
            assert same(x, want), (name, chain_rows)
            inf = plan.info()
            assert inf["chain_rows"] == {-1: -1, 0: 256}.get(chain_rows, chain_rows)
            if chain_rows == 2048 and name == "grid_rb":
                assert inf["launches"] == 1 and inf["max_level_rows"] == 1056 and inf["n_slices"] == 34


@pytest.mark.parametrize("upper", [False, True], ids=["lower", "upper"])
@pytest.mark.parametrize("name", ["grid_nat", "grid_rb", "unsorted"])
def test_the_other_triangle_of_the_same_matrix(lhpc, gpu, name, upper):
    """The grids hold both triangles: the matrix built for one solve, asked
    for the other one (its diagonal is then not the dominant one: still the
    oracle's bits, whatever their size)."""
    rp, col, val = matrix(name, upper, np.float64)
    b = rhs(rp.size - 1)
    want = sptrsv_oracle(rp, col, val, b, not upper)
    with lhpc.SpTRSVPlan(rp, col, val, upper=not upper, chain_rows=64) as plan:
        assert same(plan(dev(gpu, b)), want)


def test_int64_row_ptr(lhpc, gpu):
    rp, col, val = matrix("unsorted", False, np.float32, False, np.int64)
    assert rp.dtype == np.int64
    with lhpc.SpTRSVPlan(rp, col, val) as plan:
        assert same(plan(dev(gpu, rhs(rp.size - 1, np.float32))), solution("unsorted", False, np.float32))


# ------------------------------------------------------------------ every way in gives the same bits
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("name,chain_rows", [("mixed", 64), ("mixed_chain", 64), ("grid_rb", 2048), ("grid_nat", 0)])
def test_same_bits_through_every_entry(lhpc, gpu, name, chain_rows, dtype):
    import torch
    rp, col, val = matrix(name, False, dtype)
    n = rp.size - 1
    b, want = rhs(n, dtype), solution(name, False, dtype)
    with lhpc.SpTRSVPlan(rp, col, val, chain_rows=chain_rows) as plan:
        # host buffers, out of place and in place
        xh = plan(b)
        assert isinstance(xh, np.ndarray) and same(xh, want)
        inplace = np.array(b)
        assert plan(inplace, inplace) is inplace and same(inplace, want)
        # device buffers: current stream, a stream of its own, x aliasing b
        bd = dev(gpu, b)
        assert same(plan(bd), want)
        side = torch.cuda.Stream(gpu)
        side.wait_stream(torch.cuda.current_stream(gpu))
        xs = torch.full((n,), float("nan"), dtype=bd.dtype, device=gpu)
        plan(bd, xs, stream=side)
        side.synchronize()
        assert same(xs, want)
        alias = bd.clone()
        assert plan(alias, alias) is alias and same(alias, want)
        # captured into a graph and replayed on another right-hand side
        b2 = np.array(b[::-1])
        buf, out = dev(gpu, b), torch.full((n,), float("nan"), dtype=bd.dtype, device=gpu)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            plan(buf, out)
        buf.copy_(dev(gpu, b2))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same(out, sptrsv_oracle(rp, col, val, b2))
    # a plan from device arrays
    with lhpc.SpTRSVPlan(dev(gpu, rp), dev(gpu, col), dev(gpu, val), chain_rows=chain_rows) as plan:
        assert same(plan(bd), want)
        assert same(plan(b), want)


# ------------------------------------------------------------------ the plan info
@pytest.mark.parametrize("upper", [False, True], ids=["lower", "upper"])
@pytest.mark.parametrize("name", MATRICES)
def test_info_against_the_oracle(lhpc, gpu, name, upper):
    rp, col, val = matrix(name, upper, np.float32)
    lv, n_levels = levels_oracle(rp, col, upper)
    rows = np.bincount(lv, minlength=1)
    r = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    for unit in (False, True):
        with lhpc.SpTRSVPlan(rp, col, val, upper=upper, unit_diag=unit, chain_rows=-1) as plan:
            inf = plan.info()
        assert (inf["dtype"], inf["upper"], inf["unit_diag"], inf["n"]) == (lhpc.F32, int(upper), int(unit), rp.size - 1)
        assert inf["n_levels"] == n_levels and inf["max_level_rows"] == (rows.max() if n_levels else 0)
        assert inf["nnz"] == np.count_nonzero(col > r if upper else col < r)
        assert inf["n_slices"] == sum(-(-int(c) // 64) for c in rows) and inf["padded_entries"] >= inf["nnz"]
        assert inf["padded_entries"] % 64 == 0 and inf["device_bytes"] > 0
        assert inf["launches"] == n_levels and inf["chain_rows"] == -1  # never chain: a launch per level


@pytest.mark.parametrize("name,chain_rows,launches",
                         [("mixed", 64, 3), ("mixed", -1, 3), ("mixed", 2048, 1), ("mixed_chain", 64, 3),
                          ("mixed_chain", -1, 7), ("mixed_chain", 2048, 1), ("dense130", -1, 130), ("dense130", 0, 1),
                          ("grid_rb", 64, 2), ("grid_rb", 0, 2), ("grid_nat", 0, 1), ("diag", 64, 1), ("diag", 300, 1),
                          ("one", 0, 1), ("empty", 0, 0)])
def test_info_launches(lhpc, gpu, name, chain_rows, launches):
    """The schedule: a level above chain_rows is a grid step, a maximal run of
    levels at or below it one chain step; chain_rows < 0 is a launch per level
    (`mixed` has 3 levels, `mixed_chain` 7: tests/test_sptrsv_api.py)."""
    with lhpc.SpTRSVPlan(*matrix(name), chain_rows=chain_rows) as plan:
        assert plan.info()["launches"] == launches


# ------------------------------------------------------------------ set_values
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("name,upper,unit,chain_rows", [("unsorted", False, False, 0), ("mixed_chain", False, False, 64),
                                                         ("grid_rb", True, True, 2048), ("dense130", True, False, -1)])
def test_set_values_gives_a_fresh_plan(lhpc, gpu, name, upper, unit, chain_rows, dtype):
    rp, col, v0 = matrix(name, upper, dtype, unit)
    n = rp.size - 1
    r = np.repeat(np.arange(n), np.diff(rp))
    rng = np.random.default_rng(0x5E7)
    v1 = np.where(col == r, 3.0 + np.abs(np.asarray(v0, np.float64)), rng.uniform(-0.2, 0.2, col.size)).astype(dtype)
    bd = dev(gpu, rhs(n, dtype))
    kw = dict(upper=upper, unit_diag=unit, chain_rows=chain_rows)
    with lhpc.SpTRSVPlan(rp, col, v0, **kw) as plan, lhpc.SpTRSVPlan(rp, col, v1, **kw) as fresh:
        x0, x1 = plan(bd).clone(), fresh(bd).clone()
        assert same(x0, solution(name, upper, dtype, unit)) and not same(x0, x1)
        assert same(x1, sptrsv_oracle(rp, col, v1, rhs(n, dtype), upper, unit))
        bytes0 = plan.info()["device_bytes"]
        for val in (dev(gpu, v1), v1):  # device values, host values
            assert plan.set_values(val) is plan
            assert same(plan(bd), x1)
            plan.set_values(np.array(v0))
            assert same(plan(bd), x0)
        plan.set_values(dev(gpu, v1))
        assert plan.info()["device_bytes"] == bytes0  # only the values moved
        # a wrong nnz is refused and the plan stays as it was
        junk = dev(gpu, np.full(col.size + 1, 9.0, dtype))
        for nnz in (col.size - 1, col.size + 1):
            assert lhpc.lib.lhpc_sptrsv_plan_set_values(plan._h, junk.data_ptr(), nnz, 1, None) == -1
        assert lhpc.lib.lhpc_sptrsv_plan_set_values(plan._h, None, col.size, 1, None) == -1
        with pytest.raises(ValueError):
            plan.set_values(np.array(v0[:-1]))
        assert same(plan(bd), x1)


# ------------------------------------------------------------------ non-finite values
def _check_nonfinite(got, want, unreachable):
    got = got.cpu().numpy()
    fin = np.isfinite(want)
    assert np.all(fin[unreachable]) and np.count_nonzero(fin) > want.size // 2
    assert np.array_equal(bits(got[fin]), bits(want[fin]))  # padding was skipped, never multiplied
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    inf = np.isinf(want)
    assert np.array_equal(np.sign(got[inf]), np.sign(want[inf])) and np.count_nonzero(~fin) > 0


@pytest.mark.parametrize("chain_rows", [-1, 0])
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("what", ["inf_rhs", "zero_diagonal"])
def test_nonfinite_reaches_only_dependent_rows(lhpc, gpu, what, dtype, chain_rows):
    """grid_nat (37 × 29, lower) with b = inf at the interior cell (18, 14), or
    with that row's diagonal 0: only the cells to its right and above it can
    depend on it.  Where the oracle is finite the bits are equal; elsewhere
    the class and the sign of infinities."""
    rp, col, val = matrix("grid_nat", False, dtype)
    n, r = rp.size - 1, 14 * 37 + 18
    b, val = np.array(rhs(n, dtype)), np.array(val)
    if what == "inf_rhs":
        b[r] = np.inf
    else:
        val[rp[r]:rp[r + 1]][col[rp[r]:rp[r + 1]] == r] = 0.0
    i = np.arange(n)
    unreachable = ~((i % 37 >= 18) & (i // 37 >= 14))
    want = sptrsv_oracle(rp, col, val, b)
    assert not np.isfinite(want[r])
    with lhpc.SpTRSVPlan(rp, col, val, chain_rows=chain_rows) as plan:
        _check_nonfinite(plan(dev(gpu, b)), want, unreachable)


# ------------------------------------------------------------------ Gauss–Seidel, the first consumer
def test_gauss_seidel_sweeps_on_the_device(lhpc, gpu):
    """x ← sptrsv(D + L plan of the whole A; b − U·x), 60 sweeps in fp64 on the
    32 × 32 5-point operator with diagonal 4.1: ‖b − A·x‖ falls at every sweep
    and the final x agrees with the numpy restatement to 1e-12·max|x| (U's
    rows have at most two entries, so the SpMV's sum order cannot differ from
    numpy's; the tolerance only guards the family's rounding of a two-term
    fp64 sum)."""
    import torch
    (rp, col, val), (urp, ucol, uval), b = gauss_seidel_problem()
    xs_want, res_want = gauss_seidel_oracle()
    bd = dev(gpu, b)
    with lhpc.SpTRSVPlan(rp, col, val) as solve, lhpc.SpMVPlan(urp, ucol, uval, rp.size - 1) as upper, \
            lhpc.SpMVPlan(rp, col, val, rp.size - 1) as whole:
        x, res = torch.zeros_like(bd), []
        for _ in range(60):
            t = bd - upper(x)
            x = solve(t, t)
            res.append(torch.linalg.vector_norm(bd - whole(x)))
        res = [float(v) for v in res]
    print("gauss-seidel on the device: residual %.4g -> %.4g (numpy %.4g -> %.4g)"
          % (res[0], res[-1], res_want[0], res_want[-1]))
    assert all(r1 < r0 for r0, r1 in zip(res, res[1:]))
    got = x.cpu().numpy()
    assert np.abs(got - xs_want[-1]).max() <= 1e-12 * np.abs(xs_want[-1]).max()


# ------------------------------------------------------------------ C++ and debug build
def test_cpp_sptrsv_on_gpu(gpu):
    """tests/cpp/test_sptrsv_api.cpp (built by tests/cpp/sptrsv.mk): host flat
    arrays and device pointers against a C++ restatement, bit for bit."""
    r = subprocess.run([build_cpp()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sptrsv cpp api: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def test_debug_build_solves_trap_free(gpu):
    """grid_rb, mixed and mixed_chain under the debug library (device bounds traps on the
    plan-built indices, a synchronous check after every launch), in a child
    process as tests/test_debug_build.py does; valid inputs only."""
    from tests.test_debug_build import DEBUG_SO
    env = dict(os.environ, LHPC_LIB_PATH=DEBUG_SO)
    r = subprocess.run([sys.executable, os.path.join(S.ROOT, "tests", "debug_sptrsv_check.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DEBUG SPTRSV OK" in r.stdout
