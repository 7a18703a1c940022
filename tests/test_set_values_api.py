"""lhpc_spmv_plan_set_values / lhpc_spmm_plan_set_values ("same structure, new
values") at the boundaries that need no GPU: the symbols are exported and
mirrored, bad arguments are LHPC_ERR_INVALID_ARG before any device is touched,
the Python wrappers reject a wrong dtype or size before the C call, and the
C++ header's set_values overloads compile and link (tests/cpp/
test_set_values_api.cpp; run on the GPU by tests/test_gpu_set_values.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests._support import ROOT

NAMES = ("lhpc_spmv_plan_set_values", "lhpc_spmm_plan_set_values")
CPP_DIR = os.path.join(ROOT, "tests", "cpp")
CPP_BIN = os.path.join(CPP_DIR, "_build", "test_set_values_api")


def build_cpp():
    subprocess.run(["make", "-C", CPP_DIR, "-f", "set_values.mk"], check=True, capture_output=True)
    return CPP_BIN


def test_symbols_exported_and_mirrored(lhpc):
    from tests.test_abi import declared_functions
    declared = declared_functions()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "libhpc_amd", "_lib", "liblhpc.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for n in NAMES:
        assert n in declared, f"{n} not declared in include/lhpc.h"
        assert n in lhpc.ABI_SYMBOLS
        assert n in exported
        assert getattr(lhpc.lib, n).argtypes is not None
    assert callable(lhpc.SpMVPlan.set_values) and callable(lhpc.SpMMPlan.set_values)


@pytest.mark.parametrize("name", NAMES)
def test_invalid_arguments_without_a_device(lhpc, name):
    """Null plan, and null val with nnz > 0 (a plan cannot exist without a
    device, so the two are tested together too): LHPC_ERR_INVALID_ARG, host
    and device values alike, before any HIP call."""
    fn = getattr(lhpc.lib, name)
    v = np.ones(4, dtype=np.float32)
    for on_device in (0, 1):
        assert fn(None, v.ctypes.data, 4, on_device, None) == -1
        assert fn(None, None, 4, on_device, None) == -1
        assert fn(None, None, 0, on_device, None) == -1


class _NoCall:
    """Stands in for the C entry point: the wrapper must raise before calling it."""

    def __call__(self, *a):
        raise AssertionError("the C function was called")


@pytest.mark.parametrize("cls", ["SpMVPlan", "SpMMPlan"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_python_wrappers_reject_before_the_c_call(lhpc, monkeypatch, cls, dt):
    """A plan object without a device behind it (no constructor run): wrong
    dtype → TypeError, wrong size or shape → ValueError, other objects →
    TypeError, each naming what was expected, with the C function never called."""
    import torch
    plan = getattr(lhpc, cls).__new__(getattr(lhpc, cls))
    plan.dtype, plan.np_dtype, plan.nnz = (lhpc.F32 if dt == np.float32 else lhpc.F64), np.dtype(dt), 10
    plan._h = C.c_void_p()
    monkeypatch.setattr(lhpc.lib, "lhpc_spmv_plan_set_values", _NoCall())
    monkeypatch.setattr(lhpc.lib, "lhpc_spmm_plan_set_values", _NoCall())
    other = np.float64 if dt == np.float32 else np.float32
    with pytest.raises(TypeError, match="expected dtype"):
        plan.set_values(np.zeros(10, dtype=other))
    with pytest.raises(TypeError, match="expected dtype"):
        plan.set_values(np.zeros(10, dtype=np.int32))
    with pytest.raises(ValueError, match="expected 10 values"):
        plan.set_values(np.zeros(9, dtype=dt))
    with pytest.raises(ValueError, match="expected 10 values"):
        plan.set_values(np.zeros(11, dtype=dt))
    with pytest.raises(ValueError, match="expected 10 values"):
        plan.set_values(np.zeros((5, 2), dtype=dt))
    with pytest.raises(TypeError, match="numpy array or torch tensor"):
        plan.set_values([0.0] * 10)
    with pytest.raises(TypeError, match="expected dtype"):
        plan.set_values(torch.zeros(10, dtype=torch.float64 if dt == np.float32 else torch.float32))
    with pytest.raises(ValueError, match="plan's device"):  # host values come as numpy
        plan.set_values(torch.zeros(10, dtype=torch.float32 if dt == np.float32 else torch.float64))
    plan._h = None  # nothing to destroy


def test_cpp_header_compiles_and_links():
    """include/sparse/SpMV.hpp and SpMM.hpp: both set_values overloads of both
    plan classes, for float and double and 32- and 64-bit row offsets, in a
    stand-alone program built by tests/cpp/set_values.mk with -Wall -Wextra."""
    exe = build_cpp()
    assert os.path.exists(exe)
    out = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert n in out, f"the program does not call {n}"
