"""lhpc_bicgstab_solve at the boundaries that need no GPU: the symbol is
declared, exported and mirrored; every argument error is LHPC_ERR_INVALID_ARG
with a null plan, before any device is touched; the C++ header surface
compiles and links (tests/cpp/test_bicgstab_api.cpp, run on the GPU by
tests/test_gpu_bicgstab.py).

The test matrix and the CPU oracle of the solver live here and are checked
here: `convdiff_2d`, the 5-point upwind convection–diffusion operator (not
symmetric, so CG does not apply), and `bicgstab_oracle`, a numpy fp64
restatement of the recurrence include/lhpc.h states, with the device latch
(`latch=True`, what the library does) and without it (the plain loop that
tests only every check_every iterations and runs on past convergence)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests._support import ROOT

NAME = "lhpc_bicgstab_solve"
CPP_DIR = os.path.join(ROOT, "tests", "cpp")
CPP_BIN = os.path.join(CPP_DIR, "_build", "test_bicgstab_api")


def build_cpp():
    subprocess.run(["make", "-C", CPP_DIR, "-f", "bicgstab.mk"], check=True, capture_output=True)
    return CPP_BIN


def convdiff_2d(nx, ny, shift=0.5, dtype=np.float64):
    """(row_ptr int32, col_idx int32, val) of the upwind convection–diffusion
    operator on an nx × ny grid, cell (ix, iy) at index iy·nx + ix: diagonal
    4 + shift, west −1 − 0.5, east −1 + 0.5, south −1 − 0.25, north −1 + 0.25;
    neighbours outside the grid are dropped.  Columns ascending in each row."""
    n = nx * ny
    i = np.arange(n)
    ix, iy = i % nx, i // nx
    entries = [(i[iy > 0], i[iy > 0] - nx, -1.25), (i[ix > 0], i[ix > 0] - 1, -1.5), (i, i, 4.0 + shift),
               (i[ix < nx - 1], i[ix < nx - 1] + 1, -0.5), (i[iy < ny - 1], i[iy < ny - 1] + nx, -0.75)]
    rows = np.concatenate([e[0] for e in entries])
    cols = np.concatenate([e[1] for e in entries])
    vals = np.concatenate([np.full(e[0].size, e[2]) for e in entries])
    order = np.lexsort((cols, rows))
    rp = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return rp, cols[order].astype(np.int32), vals[order].astype(dtype)


def csr_dense(rp, col, val):
    n = rp.size - 1
    a = np.zeros((n, n))
    a[np.repeat(np.arange(n), np.diff(rp)), col] = np.asarray(val, dtype=np.float64)
    return a


def csr_matvec(rp, col, val, x):
    """A·x in fp64, each row summed in CSR order (no duplicates in a row here)."""
    prod = np.asarray(val, dtype=np.float64) * np.asarray(x, dtype=np.float64)[col]
    return np.add.reduceat(np.append(prod, 0.0), rp[:-1]) * (np.diff(rp) > 0)


def bicgstab_oracle(rp, col, val, b, x0=None, tol=1e-8, max_iter=1000, check_every=1, latch=True):
    """(x, iterations, ‖r‖/‖b‖, broke_down) by the recurrence of include/lhpc.h
    lhpc_bicgstab_solve in fp64.  latch=True: convergence and breakdown are
    tested where each scalar comes into being, as the library's device latch
    does, so check_every plays no part.  latch=False: the loop of a solver
    without the latch — rr is looked at only every check_every iterations
    and at max_iter, and the iterations in between run whatever rr is."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    mv = lambda u: csr_matvec(rp, col, val, u)  # noqa: E731
    bb = float(b @ b)
    den = np.sqrt(bb if bb > 0 else 1.0)
    stop = tol * tol * (bb if bb > 0 else 1.0)
    r = b - mv(x)
    rh, p = r.copy(), r.copy()
    rho = rr = float(r @ r)
    res = lambda q: float(np.sqrt(max(q, 0.0)) / den) if np.isfinite(q) else float(q)  # noqa: E731
    if not np.isfinite(rr):
        return x, 0, res(rr), True
    if rr <= stop:
        return x, 0, res(rr), False
    with np.errstate(all="ignore"):
        for it in range(1, max_iter + 1):
            v = mv(p)
            sigma = float(rh @ v)
            alpha = rho / sigma if sigma != 0 else np.inf * (rho if rho != 0 else np.nan)
            if latch and (not np.isfinite(sigma) or not np.isfinite(alpha) or sigma == 0):
                return x, it - 1, res(rr), True
            s = r - alpha * v
            ss = float(s @ s)
            t = mv(s)
            ts, tt = float(t @ s), float(t @ t)
            final = latch and ss <= stop
            if final:
                omega = 0.0
            else:
                omega = ts / tt if tt != 0 else np.inf * (ts if ts != 0 else np.nan)
                if latch and (not np.isfinite(tt) or not np.isfinite(omega) or omega == 0):
                    return x, it - 1, res(rr), True
            x = x + (alpha * p + omega * s)
            r = s - omega * t
            rho1, rr = float(rh @ r), float(r @ r)
            if latch:
                if not np.isfinite(rr):
                    return x, it, res(rr), True
                if rr <= stop or final:
                    return x, it, res(rr), False
                if rho1 == 0:
                    return x, it, res(rr), True
            elif it % check_every == 0 or it == max_iter:
                if not np.isfinite(rr):
                    return x, it, res(rr), True
                if rr <= stop:
                    return x, it, res(rr), False
            beta = (rho1 / rho) * (alpha / omega) if rho != 0 and omega != 0 else np.nan
            p = r + beta * (p - omega * v)
            rho = rho1
    return x, max_iter, res(rr), False


SKEW = (np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, -1.0]))  # [[0, 1], [−1, 0]]


# ------------------------------------------------------------------ the oracle itself
def test_matrix_is_the_stated_operator():
    rp, col, val = convdiff_2d(4, 3, shift=0.5)
    a = csr_dense(rp, col, val)
    assert np.diff(rp).max() == 5 and np.all(np.diag(a) == 4.5)
    i = 1 * 4 + 1  # an interior cell
    assert (a[i, i - 1], a[i, i + 1], a[i, i - 4], a[i, i + 4]) == (-1.5, -0.5, -1.25, -0.75)
    assert a[3, 4] == 0 and a[4, 3] == 0  # no wrap-around between grid rows
    assert not np.array_equal(a, a.T)
    x = np.random.default_rng(1).uniform(-1, 1, 12)
    assert np.allclose(csr_matvec(rp, col, val, x), a @ x, rtol=0, atol=1e-14)


@pytest.mark.parametrize("shape,iters", [((7, 1), 7), ((12, 9), None)])
def test_oracle_against_a_direct_solve(shape, iters):
    rp, col, val = convdiff_2d(*shape)
    n = rp.size - 1
    b = np.random.default_rng(n).uniform(-1, 1, n)
    want = np.linalg.solve(csr_dense(rp, col, val), b)
    x, it, res, broke = bicgstab_oracle(rp, col, val, b, tol=1e-10, max_iter=500)
    assert not broke and res <= 1e-10 and 0 < it <= 4 * n
    if iters is not None:
        assert it == iters
    true_res = np.linalg.norm(b - csr_matvec(rp, col, val, x)) / np.linalg.norm(b)
    assert true_res <= 2e-10
    assert np.linalg.norm(x - want) <= 1e-8 * np.linalg.norm(want)
    # the latch makes check_every irrelevant: same answer, to the bit
    x50, it50, res50, _ = bicgstab_oracle(rp, col, val, b, tol=1e-10, max_iter=500, check_every=50)
    assert it50 == it and res50 == res and np.array_equal(x50, x)


def test_oracle_without_the_latch_runs_past_convergence_into_nan():
    """What the latch is for: a 7 × 1 system converges in 7 iterations; a loop
    that looks at rr only every 50 iterations runs on, and 0/0 turns the
    solved system into a reported breakdown."""
    rp, col, val = convdiff_2d(7, 1)
    b = np.random.default_rng(7).uniform(-1, 1, 7)
    x, it, res, broke = bicgstab_oracle(rp, col, val, b, tol=1e-10, max_iter=200, check_every=50, latch=False)
    assert broke and not np.isfinite(res) and not np.isfinite(x).all()
    x, it, res, broke = bicgstab_oracle(rp, col, val, b, tol=1e-10, max_iter=200, check_every=50, latch=True)
    assert not broke and it == 7 and np.isfinite(x).all()


@pytest.mark.parametrize("x0", [(0.0, 0.0), (0.25, -0.5)])
def test_oracle_breaks_down_on_a_skew_symmetric_matrix(x0):
    """[[0, 1], [−1, 0]], b = (1, 1): r̂·v = rᵀ·A·r = r0·r1 − r1·r0 = 0 exactly for
    every r (x0 = 0: 1 − 1; x0 = (0.25, −0.5): r = (1.5, 1.25), 1.875 − 1.875),
    so α = ρ/0.  Without the latch the result is not finite; with it the
    breakdown is reported at 0 iterations with x0 untouched."""
    b = np.array([1.0, 1.0])
    x, it, res, broke = bicgstab_oracle(*SKEW, b, x0=x0, max_iter=5, latch=False)
    assert broke and not np.isfinite(res) and not np.isfinite(x).any()
    x, it, res, broke = bicgstab_oracle(*SKEW, b, x0=x0, max_iter=5, latch=True)
    assert broke and it == 0 and np.isfinite(res) and np.array_equal(x, np.array(x0))


# ------------------------------------------------------------------ the symbol
def test_symbol_exported_and_mirrored(lhpc):
    from tests.test_abi import declared_functions
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "libhpc_amd", "_lib", "liblhpc.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert NAME in declared_functions(), f"{NAME} not declared in include/lhpc.h"
    assert NAME in lhpc.ABI_SYMBOLS and NAME in exported
    assert getattr(lhpc.lib, NAME).argtypes == lhpc.lib.lhpc_cg_solve.argtypes  # shaped like lhpc_cg_solve
    assert callable(lhpc.bicgstab) and "bicgstab" in lhpc.__all__
    import inspect
    assert str(inspect.signature(lhpc.bicgstab)) == str(inspect.signature(lhpc.cg))


# ------------------------------------------------------------------ argument checks, no device
def _call(lhpc, plan=None, b=1, x=1, tol=1e-8, max_iter=10, check_every=1):
    buf = np.zeros(4)
    it, res = C.c_int(-5), C.c_double(-5.0)
    st = lhpc.lib.lhpc_bicgstab_solve(plan, buf.ctypes.data if b else None, buf.ctypes.data if x else None, tol,
                                      max_iter, check_every, C.byref(it), C.byref(res), None)
    assert (it.value, res.value) == (-5, -5.0)  # a refused call writes no output
    return st


@pytest.mark.parametrize("bad", [dict(), dict(b=0), dict(x=0), dict(max_iter=-1), dict(tol=-1e-30),
                                 dict(tol=float("nan")), dict(tol=-float("inf"))])
def test_invalid_arguments_with_a_null_plan(lhpc, bad):
    assert _call(lhpc, plan=None, **bad) == -1


@pytest.mark.parametrize("bad", [dict(b=0), dict(x=0), dict(max_iter=-1), dict(tol=-1.0), dict(tol=float("nan"))])
def test_invalid_arguments_come_before_the_plan_is_read(lhpc, bad):
    """With a plan pointer that cannot be read (address 8): the argument
    errors are returned without touching it."""
    assert _call(lhpc, plan=C.c_void_p(8), **bad) == -1


def test_python_wrapper_rejects_host_tensors_before_the_c_call(lhpc, monkeypatch):
    import torch

    def no_call(*a):
        raise AssertionError("the C function was called")

    monkeypatch.setattr(lhpc.lib, NAME, no_call)
    plan = lhpc.SpMVPlan.__new__(lhpc.SpMVPlan)
    plan._h = None
    with pytest.raises(ValueError, match="device tensors"):
        lhpc.bicgstab(plan, torch.zeros(3, dtype=torch.float64))


def test_cpp_header_compiles_and_links():
    """sparse::bicgstab of include/sparse/SpMV.hpp for float and double in a
    stand-alone program built by tests/cpp/bicgstab.mk with -Wall -Wextra."""
    exe = build_cpp()
    assert os.path.exists(exe)
    out = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True, check=True).stdout
    assert NAME in out, f"the program does not call {NAME}"
