"""lhpc_sptrsv_* at the boundaries that need no GPU: the six symbols are
declared, exported and mirrored; every argument error is LHPC_ERR_INVALID_ARG
before any device is touched; LHPC_PLAN_TRANSPOSE is LHPC_ERR_UNSUPPORTED; the
info struct mirror matches the header; lhpc_sptrsv_levels equals the level
rule on every test matrix and refuses invalid ones; the C++ header surface
compiles and links (tests/cpp/test_sptrsv_api.cpp, run on the GPU by
tests/test_gpu_sptrsv.py).

The test matrices and the CPU oracles live here and are checked here:
`sptrsv_oracle`, a plain Python loop restating include/lhpc.h "CSR triangular
solve" (fp64 scalars, the final cast to the dtype), and `levels_oracle`, the
level rule.  Every matrix is made diagonally dominant inside the triangle
under test (d_i = 2 + Σ|off-diagonal|, off-diagonals U[−1, 1) from
gen_values), so |x| ≤ max|b| and nothing overflows; with a unit diagonal the
off-diagonals are divided by that d_i instead (|x| ≤ max|b|·(1 + max Σ|off-diagonal|/2),
test_oracle_against_a_direct_solve) and the stored diagonal entries are set
to 7, which the solve must ignore."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests._support import ROOT

NAMES = ("lhpc_sptrsv_levels", "lhpc_sptrsv_plan_create", "lhpc_sptrsv", "lhpc_sptrsv_plan_set_values",
         "lhpc_sptrsv_plan_info_get", "lhpc_sptrsv_plan_destroy")
CPP_DIR = os.path.join(ROOT, "tests", "cpp")
CPP_BIN = os.path.join(CPP_DIR, "_build", "test_sptrsv_api")
MATRICES = ("grid_nat", "grid_rb", "dense130", "mixed", "mixed_chain", "diag", "unsorted", "one", "empty")


def build_cpp():
    subprocess.run(["make", "-C", CPP_DIR, "-f", "sptrsv.mk"], check=True, capture_output=True)
    return CPP_BIN


# ------------------------------------------------------------------ the oracles
def kept(upper, i, c):
    return c > i if upper else c < i


def levels_oracle(rp, col, upper=False):
    """(level, n_levels): 0 for a row without kept off-diagonal entries, else
    1 + the highest level among the rows it depends on."""
    n = rp.size - 1
    level = np.zeros(n, dtype=np.int32)
    for i in (range(n - 1, -1, -1) if upper else range(n)):
        deps = [int(level[c]) + 1 for c in col[rp[i]:rp[i + 1]] if kept(upper, i, c)]
        level[i] = max(deps, default=0)
    return level, int(level.max()) + 1 if n else 0


def sptrsv_oracle(rp, col, val, b, upper=False, unit=False):
    """x by the arithmetic of include/lhpc.h: per row, in CSR order,
    s += (double)val·(double)x[col] (a Python float is an IEEE double and
    rounds the product before the add), then x_i = T((b_i − s) / d_i)."""
    n = rp.size - 1
    x = np.zeros(n, dtype=val.dtype)
    with np.errstate(all="ignore"):
        for i in (range(n - 1, -1, -1) if upper else range(n)):
            s, d = 0.0, np.float64(1.0)
            for p in range(rp[i], rp[i + 1]):
                c = col[p]
                if c == i:
                    if not unit:
                        d = np.float64(val[p])
                elif kept(upper, i, c):
                    s = s + float(val[p]) * float(x[c])
            r = np.float64(float(b[i]) - s)
            x[i] = val.dtype.type(r if unit else r / d)
    return x


# ------------------------------------------------------------------ the matrices
def _grid_coo(nx, ny, index):
    """5-point pattern (diagonal and the four neighbours) on nx × ny, cell
    (ix, iy) at row index[iy·nx + ix]."""
    i = np.arange(nx * ny)
    ix, iy = i % nx, i // nx
    pairs = [(i[iy > 0], i[iy > 0] - nx), (i[ix > 0], i[ix > 0] - 1), (i, i),
             (i[ix < nx - 1], i[ix < nx - 1] + 1), (i[iy < ny - 1], i[iy < ny - 1] + nx)]
    return index[np.concatenate([p[0] for p in pairs])], index[np.concatenate([p[1] for p in pairs])]


def red_black_index(nx, ny):
    """cell → row: the cells with even ix + iy first, then the odd ones."""
    i = np.arange(nx * ny)
    order = np.argsort((i % nx + i // nx) % 2, kind="stable")
    index = np.empty(nx * ny, dtype=np.int64)
    index[order] = i
    return index


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(n, rows, cols, shuffled) of a LOWER test matrix as coordinates."""
    rng = np.random.default_rng(0x7A5)
    if name in ("grid_nat", "unsorted"):
        r, c = _grid_coo(37, 29, np.arange(37 * 29))
        if name == "unsorted":  # one off-diagonal coordinate twice: (500, 499)
            r, c = np.append(r, 500), np.append(c, 499)
        return 37 * 29, r, c, name == "unsorted"
    if name == "grid_rb":
        r, c = _grid_coo(64, 33, red_black_index(64, 33))
        return 64 * 33, r, c, False
    if name == "dense130":
        r, c = np.tril_indices(130)
        return 130, r, c, False
    if name in ("mixed", "mixed_chain"):
        # 1500 independent rows; 5 rows each depending on the one before —
        # `mixed`: on a row of the block before (row i − 5), so the five are one
        # level and the matrix has 3 (the launch counts asked of it, 3 / 3 / 1 at
        # chain_rows 64 / −1 / 2048, hold for this reading only); `mixed_chain`:
        # on the row just before (i − 1), five levels of one row, 7 in all —
        # then 1500 rows depending on three of the first block and on row 1504
        a = np.arange(1500, 1505)
        t = np.arange(1505, 3005)
        i = np.arange(3005)
        r = np.concatenate([i, a, np.repeat(t, 4)])
        dep = np.concatenate([np.sort(rng.choice(1500, 3, replace=False)) for _ in t]).reshape(-1, 3)
        back = 5 if name == "mixed" else 1
        c = np.concatenate([i, a - back, np.column_stack([dep, np.full(t.size, 1504)]).ravel()])
        return 3005, r, c, False
    n = {"diag": 200, "one": 1, "empty": 0}[name]
    return n, np.arange(n), np.arange(n), False


@functools.lru_cache(maxsize=None)
def matrix(name, upper=False, dtype=np.float64, unit=False, rp_dtype=np.int32):
    """(row_ptr, col_idx, val) of a test matrix; `upper`: its transpose.  The
    grids and `unsorted` hold both triangles (the other one is to be ignored)."""
    n, r, c, shuffled = pattern(name)
    if upper:
        r, c = c, r
    rng = np.random.default_rng(0x51)
    key = rng.permutation(r.size) if shuffled else c
    order = np.lexsort((key, r))
    r, c = r[order], c[order]
    rp = np.zeros(n + 1, dtype=rp_dtype)
    np.cumsum(np.bincount(r, minlength=n), out=rp[1:])
    import libhpc_amd as L
    val = L.gen_values(np.float64, 0, r.size, L.SEED_A).astype(np.float64)
    k = (c > r) if upper else (c < r)
    d = 2.0 + np.bincount(r[k], weights=np.abs(val[k]), minlength=n)
    if unit:
        val[k] /= d[r[k]]
        val[c == r] = 7.0
    else:
        val[c == r] = d[r[c == r]]
    out = (rp, c.astype(np.int32), val.astype(dtype))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rhs(n, dtype=np.float64):
    import libhpc_amd as L
    b = L.gen_values(dtype, 0, n, L.SEED_X)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def solution(name, upper=False, dtype=np.float64, unit=False):
    """The oracle's x for the matrix and rhs(n, dtype), computed once."""
    rp, col, val = matrix(name, upper, dtype, unit)
    x = sptrsv_oracle(rp, col, val, rhs(rp.size - 1, dtype), upper, unit)
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------ the oracles and matrices themselves
def test_matrices_are_what_they_claim():
    lv, nl = levels_oracle(*matrix("grid_nat")[:2])
    assert nl == 65 and np.bincount(lv).max() == 29 and np.bincount(lv).min() == 1
    lv, nl = levels_oracle(*matrix("grid_rb")[:2])
    assert nl == 2 and list(np.bincount(lv)) == [1056, 1056]
    rp, col, _ = matrix("dense130")
    lv, nl = levels_oracle(rp, col)
    assert nl == 130 and list(lv) == list(range(130)) and list(np.diff(rp)) == list(range(1, 131))
    lv, nl = levels_oracle(*matrix("mixed")[:2])
    assert nl == 3 and list(np.bincount(lv)) == [1500, 5, 1500]
    lv, nl = levels_oracle(*matrix("mixed_chain")[:2])
    assert nl == 7 and list(np.bincount(lv)) == [1500, 1, 1, 1, 1, 1, 1500]
    assert levels_oracle(*matrix("diag")[:2])[1] == 1 and levels_oracle(*matrix("empty")[:2])[1] == 0
    rp, col, _ = matrix("unsorted")
    assert any(np.any(np.diff(col[rp[i]:rp[i + 1]]) < 0) for i in range(rp.size - 1))  # rows not sorted
    row = col[rp[500]:rp[501]]
    assert np.count_nonzero(row == 499) == 2 and np.any(row > 500)  # the duplicate, and the other triangle
    # the transposes have as many levels (row 1499 now ends the chain; the
    # first block's other rows sit at level 0 or 1)
    lv_u, nl_u = levels_oracle(*matrix("mixed_chain", upper=True)[:2], upper=True)
    assert nl_u == 7 and list(np.bincount(lv_u)[2:]) == [1, 1, 1, 1, 1] and lv_u[1499] == 6
    lv_u, nl_u = levels_oracle(*matrix("mixed", upper=True)[:2], upper=True)
    assert nl_u == 3 and lv_u[1504] == 1 and lv_u[1499] == 2 and np.count_nonzero(lv_u == 2) == 1


@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("upper", [False, True])
def test_oracle_against_a_direct_solve(upper, unit):
    """On the dense triangle in fp64, to 1e-12 relative."""
    rp, col, val = matrix("dense130", upper, np.float64, unit)
    a = np.zeros((130, 130))
    a[np.repeat(np.arange(130), np.diff(rp)), col] = val
    if unit:
        np.fill_diagonal(a, 1.0)
    b = rhs(130)
    want = np.linalg.solve(a, b)
    got = solution("dense130", upper, np.float64, unit)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # diagonal dominance: nothing grows.  Non-unit: |x_i| ≤ (|b_i| + S_i·max|x|) / (2 + S_i) with S_i = Σ|off-diagonal|,
    # so |x| ≤ max|b|; unit (off-diagonals divided by 2 + S_i): |x_i| ≤ |b_i| + S_i/(2 + S_i)·max|x|, so
    # |x| ≤ max|b|·(1 + max S/2)
    off = np.abs(a - np.diag(np.diag(a))).sum(axis=1).max()
    assert np.abs(got).max() <= np.abs(b).max() * (1.0 + (off / (1.0 - off) if unit else 0.0))


def test_oracle_ignores_the_other_triangle_and_keeps_duplicates():
    """`unsorted` is grid_nat with (500, 499) twice: the lower solve differs
    from grid_nat's only through that entry, the upper triangle plays no part."""
    rp, col, val = matrix("unsorted")
    b = rhs(rp.size - 1)
    x = sptrsv_oracle(rp, col, val, b)
    low = np.repeat(np.arange(rp.size - 1), np.diff(rp)) >= col
    rp2 = np.zeros_like(rp)
    np.cumsum(np.add.reduceat(low.astype(np.int64), rp[:-1]), out=rp2[1:])
    assert np.array_equal(sptrsv_oracle(rp2, col[low], val[low], b), x)
    a = np.zeros((rp.size - 1,) * 2)
    np.add.at(a, (np.repeat(np.arange(rp.size - 1), np.diff(rp))[low], col[low]), val[low])  # duplicates summed
    assert np.abs(x - np.linalg.solve(a, b)).max() <= 1e-12


# ------------------------------------------------------------------ Gauss–Seidel, the first consumer
@functools.lru_cache(maxsize=None)
def gauss_seidel_problem():
    """(A, U, b): the 32 × 32 5-point operator with diagonal 4.1 (fp64), its
    strict upper part and a right-hand side in U[−1, 1)."""
    from tests._support import laplacian_2d
    rp, col, val = laplacian_2d(32, 32, np.float64, 0.1)
    up = col > np.repeat(np.arange(rp.size - 1), np.diff(rp))
    urp = np.zeros_like(rp)
    np.cumsum(np.add.reduceat(np.append(up, False).astype(np.int64), rp[:-1])[:rp.size - 1], out=urp[1:])
    return (rp, col, val), (urp, col[up], val[up]), rhs(rp.size - 1)


def csr_matvec(rp, col, val, x):
    """A·x in fp64, each row summed in CSR order from 0.0."""
    y = np.zeros(rp.size - 1)
    for i in range(rp.size - 1):
        s = 0.0
        for p in range(rp[i], rp[i + 1]):
            s = s + float(val[p]) * float(x[col[p]])
        y[i] = s
    return y


@functools.lru_cache(maxsize=None)
def gauss_seidel_oracle(sweeps=60):
    """(x after every sweep, ‖b − A·x‖ after every sweep) of
    x ← (D + L)⁻¹·(b − U·x) from x = 0, the solve by sptrsv_oracle on the whole A."""
    a, u, b = gauss_seidel_problem()
    x, xs, res = np.zeros(b.size), [], []
    for _ in range(sweeps):
        x = sptrsv_oracle(*a, b - csr_matvec(*u, x))
        xs.append(x)
        res.append(float(np.linalg.norm(b - csr_matvec(*a, x))))
    return xs, res


def test_gauss_seidel_restatement_converges():
    (rp, col, val), (urp, ucol, uval), b = gauss_seidel_problem()
    assert np.all(val[col == np.repeat(np.arange(1024), np.diff(rp))] == 4.1) and np.diff(urp).max() == 2
    assert np.all(uval == -1.0) and ucol.size == 2 * 32 * 31
    _, res = gauss_seidel_oracle()
    print("gauss-seidel residuals: first %.4g last %.4g" % (res[0], res[-1]))
    assert all(r1 < r0 for r0, r1 in zip(res, res[1:]))  # falls at every sweep
    assert res[-1] < 0.01 * res[0]


# ------------------------------------------------------------------ the symbols
def test_symbols_exported_and_mirrored(lhpc):
    from tests.test_abi import declared_functions
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "libhpc_amd", "_lib", "liblhpc.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NAMES:
        assert name in declared_functions(), f"{name} not declared in include/lhpc.h"
        assert name in lhpc.ABI_SYMBOLS and name in exported
        assert getattr(lhpc.lib, name).argtypes is not None
    for name in ("SpTRSVPlan", "SpTRSVPlanInfo", "sptrsv_levels", "TRSV_UPPER", "TRSV_UNIT_DIAG"):
        assert name in lhpc.__all__ and hasattr(lhpc, name)
    assert (lhpc.TRSV_LOWER, lhpc.TRSV_UPPER, lhpc.TRSV_UNIT_DIAG) == (0, 1, 2)
    import inspect
    sig = inspect.signature(lhpc.SpTRSVPlan.__init__).parameters
    assert [(k, v.default) for k, v in sig.items()][4:] == [("upper", False), ("unit_diag", False), ("chain_rows", 0),
                                                            ("flags", 0), ("device", None)]
    assert list(sig)[:4] == ["self", "row_ptr", "col_idx", "val"]
    assert list(inspect.signature(lhpc.SpTRSVPlan.__call__).parameters) == ["self", "b", "x", "stream"]
    assert list(inspect.signature(lhpc.sptrsv_levels).parameters) == ["row_ptr", "col_idx", "upper", "unit_diag"]
    for m in ("__call__", "info", "set_values", "close", "__enter__", "__exit__"):
        assert callable(getattr(lhpc.SpTRSVPlan, m))


def test_info_struct_mirror_matches_header(lhpc, tmp_path):
    """Size and every field offset of lhpc_sptrsv_plan_info against a probe
    compiled from include/lhpc.h (the method of tests/test_abi.py)."""
    cls = lhpc.SpTRSVPlanInfo
    fields = [f[0] for f in cls._fields_]
    assert fields == ["dtype", "device", "upper", "unit_diag", "n", "nnz", "n_levels", "max_level_rows", "n_slices",
                      "padded_entries", "chain_rows", "launches", "device_bytes"]
    src = tmp_path / "probe.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"lhpc.h\"\nint main(void){\n"
                   "printf(\"size %zu\\n\", sizeof(lhpc_sptrsv_plan_info));\n"
                   + "".join(f"printf(\"{n} %zu\\n\", offsetof(lhpc_sptrsv_plan_info, {n}));\n" for n in fields)
                   + "printf(\"flags %d %d %d\\n\", LHPC_TRSV_LOWER, LHPC_TRSV_UPPER, LHPC_TRSV_UNIT_DIAG);\n"
                   + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    got = dict(l.split() for l in lines[:-1])
    assert int(got["size"]) == C.sizeof(cls)
    for n in fields:
        assert int(got[n]) == getattr(cls, n).offset, n
    assert lines[-1] == "flags 0 1 2"


# ------------------------------------------------------------------ argument checks, no device
def _create(lhpc, **kw):
    a = dict(out=True, dtype=1, n=2, nnz=3, row_ptr=np.array([0, 1, 3], np.int32), bits=32,
             col=np.array([0, 0, 1], np.int32), val=np.array([2.0, 1.0, 2.0]), trsv=0, chain_rows=0, device=-1, flags=0)
    a.update(kw)
    h = C.c_void_p(0x5A)
    ptr = lambda v: v.ctypes.data if v is not None else None  # noqa: E731
    st = lhpc.lib.lhpc_sptrsv_plan_create(C.byref(h) if a["out"] else None, a["dtype"], a["n"], a["nnz"],
                                          ptr(a["row_ptr"]), a["bits"], ptr(a["col"]), ptr(a["val"]), a["trsv"],
                                          a["chain_rows"], a["device"], a["flags"])
    return st, h


INVALID = [dict(out=False), dict(row_ptr=None), dict(col=None), dict(val=None), dict(dtype=2), dict(dtype=-1),
           dict(bits=16), dict(n=-1), dict(nnz=-1), dict(n=2**31), dict(trsv=4), dict(trsv=1 << 31),
           dict(flags=1 << 4), dict(flags=1 << 10), dict(flags=(1 << 11) | (1 << 5)), dict(device=-2)]


@pytest.mark.parametrize("bad", INVALID, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_create_argument_errors_come_before_the_device(lhpc, bad):
    """LHPC_ERR_INVALID_ARG whether a device is present or not (without one
    the alternative would be LHPC_ERR_NO_DEVICE), even for a matrix that is
    invalid as well (BAD_CSR comes later)."""
    st, h = _create(lhpc, **bad)
    assert st == -1
    assert not h.value or not bad.get("out", True)  # *out is cleared
    if "col" not in bad:
        assert _create(lhpc, col=np.array([0, 9, 1], np.int32), **bad)[0] == -1


def test_create_refuses_transpose_and_huge_nnz(lhpc):
    for flags in (1 << 11, (1 << 11) | 1, (1 << 11) | 2):
        st, h = _create(lhpc, flags=flags)
        assert st == -5 and not h.value
    st, h = _create(lhpc, nnz=2**32, bits=64, row_ptr=np.array([0, 1, 3], np.int64))
    assert st == -5 and not h.value


def test_create_validates_before_the_device(lhpc):
    """Host input: LHPC_ERR_BAD_CSR with or without a device."""
    assert _create(lhpc, col=np.array([0, 2, 1], np.int32))[0] == -2            # column out of range
    assert _create(lhpc, col=np.array([0, 0, 0], np.int32))[0] == -2            # row 1 without a diagonal
    assert _create(lhpc, col=np.array([0, 1, 1], np.int32))[0] == -2            # row 1 with two
    assert _create(lhpc, row_ptr=np.array([0, 4, 3], np.int32))[0] == -2        # decreasing row_ptr
    assert _create(lhpc, row_ptr=np.array([0, 1, 2], np.int32))[0] == -2        # row_ptr[n] ≠ nnz


def test_create_without_a_device_fails_loudly(lhpc):
    if lhpc.device_count() > 0:
        pytest.skip("a GPU is present")
    st, h = _create(lhpc)
    assert st == -4 and not h.value
    with pytest.raises(lhpc.LhpcError) as e:
        lhpc.SpTRSVPlan(*matrix("diag"))
    assert e.value.status == -4


def test_null_plan_calls(lhpc):
    buf = np.zeros(4)
    info = lhpc.SpTRSVPlanInfo()
    assert lhpc.lib.lhpc_sptrsv(None, buf.ctypes.data, buf.ctypes.data, 0, None) == -1
    assert lhpc.lib.lhpc_sptrsv_plan_set_values(None, buf.ctypes.data, 4, 0, None) == -1
    assert lhpc.lib.lhpc_sptrsv_plan_info_get(None, C.byref(info)) == -1
    assert lhpc.lib.lhpc_sptrsv_plan_destroy(None) == 0


# ------------------------------------------------------------------ lhpc_sptrsv_levels
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("name", MATRICES)
def test_levels_equal_the_oracle(lhpc, name, upper, unit):
    rp, col, _ = matrix(name, upper)
    want, n_want = levels_oracle(rp, col, upper)
    got, n_got = lhpc.sptrsv_levels(rp, col, upper=upper, unit_diag=unit)
    assert n_got == n_want and np.array_equal(got, want)
    # the grids hold both triangles: the same A serves the other solve
    if name in ("grid_nat", "grid_rb", "unsorted"):
        want, n_want = levels_oracle(rp, col, not upper)
        got, n_got = lhpc.sptrsv_levels(rp, col, upper=not upper, unit_diag=unit)
        assert n_got == n_want and np.array_equal(got, want)


def test_levels_int64_row_ptr_and_missing_unit_diagonal(lhpc):
    rp, col, _ = matrix("grid_nat", rp_dtype=np.int64)
    assert rp.dtype == np.int64
    want, n_want = levels_oracle(rp, col)
    got, n_got = lhpc.sptrsv_levels(rp, col)
    assert n_got == n_want and np.array_equal(got, want)
    # a unit diagonal needs no stored diagonal entries
    strict = col != np.repeat(np.arange(rp.size - 1), np.diff(rp))
    rp2 = np.zeros_like(rp)
    np.cumsum(np.add.reduceat(strict.astype(np.int64), rp[:-1]), out=rp2[1:])
    got, n_got = lhpc.sptrsv_levels(rp2, col[strict], unit_diag=True)
    assert n_got == n_want and np.array_equal(got, want)
    with pytest.raises(lhpc.LhpcError) as e:
        lhpc.sptrsv_levels(rp2, col[strict])
    assert e.value.status == -2


@pytest.mark.parametrize("bits", [32, 64])
def test_levels_refuse_invalid_matrices(lhpc, bits):
    dt = np.int32 if bits == 32 else np.int64

    def call(rp, col, trsv=0, n=None):
        rp, col = np.array(rp, dt), np.array(col, np.int32)
        n = rp.size - 1 if n is None else n
        level, nl = np.full(max(n, 1), -7, np.int32), C.c_int64(-7)
        return lhpc.lib.lhpc_sptrsv_levels(n, col.size, rp.ctypes.data, bits, col.ctypes.data, trsv,
                                           level.ctypes.data, C.byref(nl)), nl.value

    assert call([0, 1, 3], [0, 0, 1]) == (0, 2)
    assert call([0, 1, 3], [0, 0, 0])[0] == -2          # missing diagonal
    assert call([0, 1, 3], [0, 0, 0], trsv=2) == (0, 2)  # … which a unit diagonal does not need
    assert call([0, 1, 3], [0, 1, 1])[0] == -2          # doubled diagonal
    assert call([0, 1, 3], [0, 1, 1], trsv=2) == (0, 1)
    assert call([0, 1, 3], [0, 0, 2])[0] == -2          # column out of range
    assert call([0, 1, 3], [0, -1, 1])[0] == -2
    assert call([0, 1, 3], [0, 0, 2], trsv=3)[0] == -2  # … also where the triangle would ignore it
    assert call([0, 3, 1, 3], [0, 1, 2])[0] == -2       # decreasing row_ptr
    assert call([1, 1, 3], [0, 0, 1])[0] == -2          # row_ptr[0] ≠ 0
    assert call([0, 1, 2], [0, 0, 1])[0] == -2          # row_ptr[n] ≠ nnz
    assert call([0], [], n=0) == (0, 0)                 # n = 0: no levels
    assert call([0, 1, 3], [0, 0, 1], trsv=4)[0] == -1  # unknown bit
    assert call([0, 1, 3], [0, 0, 1], n=-1)[0] == -1


# ------------------------------------------------------------------ the C++ surface
def test_cpp_header_compiles_and_links():
    """sparse::SpTRSVPlan / sparse::sptrsv / sparse::sptrsv_levels of
    include/sparse/SpTRSV.hpp for float and double in a stand-alone program
    built by tests/cpp/sptrsv.mk with -Wall -Wextra."""
    exe = build_cpp()
    assert os.path.exists(exe)
    out = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert name in out, f"the program does not call {name}"
