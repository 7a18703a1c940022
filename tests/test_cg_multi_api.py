"""lhpc_spmm_dot and lhpc_cg_solve_multi (libhpc_amd.spmm_dot / cg_multi) checks
that need no GPU: both entry points are exported and bound, every size or
argument error is LHPC_ERR_INVALID_ARG before the plan is read, the Python
wrappers refuse host arrays, wrong dtypes and mismatched widths, and the new
kernels are all in the product library's code objects, without scratch,
within the register budget DESIGN.md §4.2 records for them."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests.test_kernel_resources import BUNDLER, LIB, READELF, kernels

INVALID_ARG = -1
SYMBOLS = ("lhpc_spmm_dot", "lhpc_cg_solve_multi")
# the project's floor for a gather-latency kernel (4 waves per SIMD); measured: 50–69
SPMM_DOT_VGPR_BUDGET = 128
CANARY = -1234.5


def test_symbols_exported_and_bound(lhpc):
    for n in SYMBOLS:
        assert n in lhpc.ABI_SYMBOLS
        fn = getattr(lhpc.lib, n)
        assert fn.argtypes is not None and fn.restype is C.c_int, n
    for n in ("spmm_dot", "cg_multi"):
        assert n in lhpc.__all__ and callable(getattr(lhpc, n))


def _bufs():
    return [np.full(64, CANARY, np.float32) for _ in range(3)], np.full(8, CANARY, np.float64)


@pytest.mark.parametrize("k,ldx,ldy,ldw", [(0, 4, 4, 4), (-1, 4, 4, 4), (3, 2, 4, 4), (3, 4, 2, 4), (3, 4, 4, 2),
                                           (3, -1, 4, 4), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)])
def test_spmm_dot_size_errors_come_before_the_plan_is_read(lhpc, k, ldx, ldy, ldw):
    """A zeroed stand-in for the handle is enough to reach the size checks:
    they come before the plan is read and before any HIP call."""
    stand_in = C.create_string_buffer(4096)
    (x, y, w), d = _bufs()
    assert lhpc.lib.lhpc_spmm_dot(stand_in, k, x.ctypes.data, ldx, y.ctypes.data, ldy, w.ctypes.data, ldw,
                                  d.ctypes.data, None) == INVALID_ARG
    assert all((a == CANARY).all() for a in (x, y, w, d))


@pytest.mark.parametrize("null", ["X", "Y", "W", "dots"])
def test_spmm_dot_null_pointers(lhpc, null):
    stand_in = C.create_string_buffer(4096)
    (x, y, w), d = _bufs()
    p = dict(X=x.ctypes.data, Y=y.ctypes.data, W=w.ctypes.data, dots=d.ctypes.data)
    p[null] = None
    assert lhpc.lib.lhpc_spmm_dot(stand_in, 3, p["X"], 4, p["Y"], 4, p["W"], 4, p["dots"], None) == INVALID_ARG
    assert all((a == CANARY).all() for a in (x, y, w, d))


@pytest.mark.parametrize("bad", [dict(k=0), dict(k=-2), dict(ldb=2), dict(ldx=2), dict(ldb=-1), dict(max_iter=-1),
                                 dict(tol=-1e-3), dict(tol=float("nan")), dict(B=None), dict(X=None)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_cg_solve_multi_argument_errors_come_before_the_plan_is_read(lhpc, bad):
    stand_in = C.create_string_buffer(4096)
    b = np.full(64, CANARY, np.float32)
    x = np.full(64, CANARY, np.float32)
    iters = np.full(8, -7, np.int32)
    resid = np.full(8, CANARY, np.float64)
    a = dict(k=3, B=b.ctypes.data, ldb=4, X=x.ctypes.data, ldx=4, tol=1e-8, max_iter=10)
    a.update(bad)
    st = lhpc.lib.lhpc_cg_solve_multi(stand_in, a["k"], a["B"], a["ldb"], a["X"], a["ldx"], a["tol"], a["max_iter"], 1,
                                      iters.ctypes.data, resid.ctypes.data, None)
    assert st == INVALID_ARG
    assert (b == CANARY).all() and (x == CANARY).all() and (iters == -7).all() and (resid == CANARY).all()
    assert stand_in.raw == bytes(4096), "the stand-in handle was written"


def test_null_plan_calls(lhpc):
    (x, y, w), d = _bufs()
    assert lhpc.lib.lhpc_spmm_dot(None, 1, x.ctypes.data, 1, y.ctypes.data, 1, w.ctypes.data, 1, d.ctypes.data,
                                  None) == INVALID_ARG
    assert lhpc.lib.lhpc_cg_solve_multi(None, 1, x.ctypes.data, 1, y.ctypes.data, 1, 1e-8, 10, 1, None, None,
                                        None) == INVALID_ARG


def test_python_wrapper_argument_errors(lhpc):
    """Checked before the handle is used: a stand-in plan object is enough."""
    import torch
    plan = SimpleNamespace(np_dtype=np.float32, n_rows=8, n_cols=8, _h=None)
    B = torch.ones((8, 4))
    for fn, args in ((lhpc.cg_multi, (np.ones((8, 4), np.float32),)),  # host arrays
                     (lhpc.cg_multi, (B, torch.zeros((8, 4)))),
                     (lhpc.spmm_dot, (np.ones((8, 4), np.float32), np.ones((8, 4), np.float32))),
                     (lhpc.spmm_dot, (B, B))):
        with pytest.raises(ValueError, match="device tensors"):
            fn(plan, *args)
    with pytest.raises(TypeError):  # wrong dtype
        lhpc.cg_multi(plan, B.double())
    with pytest.raises(TypeError):
        lhpc.cg_multi(plan, B, torch.zeros((8, 4), dtype=torch.float64))
    with pytest.raises(TypeError):
        lhpc.spmm_dot(plan, B.double(), B.double())
    with pytest.raises(ValueError, match="expected 4 columns"):  # X narrower than B
        lhpc.cg_multi(plan, B, torch.zeros((8, 3)))
    with pytest.raises(ValueError, match="expected 4 columns"):  # W narrower than X
        lhpc.spmm_dot(plan, B, B[:, :3])
    with pytest.raises(ValueError):
        lhpc.cg_multi(plan, B[:, ::2])  # non-unit inner stride


@pytest.fixture(scope="module")
def ks():
    import os
    if not os.path.exists(READELF) or not os.path.exists(BUNDLER) or not os.path.exists(LIB):
        pytest.skip("llvm-readelf / clang-offload-bundler or the built library not available")
    return kernels()


def _pick(ks, pat):
    return {m.group(0): r for n, r in ks.items() for m in [re.search(pat, n)] if m}


def test_every_new_instantiation_is_in_the_code_object(ks):
    """k_spmm_dot: fp32/fp64 × int32/int64 row_ptr × panel widths 4, 8, 16, 32;
    the solver's k_cgm_init / k_cgm_r / k_cgm_xp: fp32/fp64 × the four panels;
    the per-column finish."""
    want = {f"k_spmm_dotI{t}{i}Li{p}EE" for t in "fd" for i in "il" for p in (4, 8, 16, 32)}
    assert set(_pick(ks, r"k_spmm_dotI[fd][il]Li\d+EE")) == want
    for name in ("k_cgm_init", "k_cgm_r", "k_cgm_xp"):
        want = {f"{name}I{t}Li{p}EE" for t in "fd" for p in (4, 8, 16, 32)}
        assert set(_pick(ks, name + r"I[fd]Li\d+EE")) == want, name
    assert len(_pick(ks, r"k_coldot_finish")) == 1
    assert not [n for n in ks if "k_spmm_dot" in n and "k_spmm_csr" in n]


def test_new_kernels_use_no_scratch_and_stay_in_budget(ks):
    new = {n: r for n, r in ks.items() if re.search(r"k_spmm_dot|k_cgm_|k_coldot_finish", n)}
    assert len(new) == 16 + 24 + 1, sorted(new)
    for n, r in new.items():
        assert not r["vgpr_spill_count"] and not r["private_segment_fixed_size"], (n, r)
        assert not r["sgpr_spill_count"], (n, r)
        if "k_spmm_dot" in n:
            assert r["vgpr_count"] <= SPMM_DOT_VGPR_BUDGET, (n, r["vgpr_count"])
