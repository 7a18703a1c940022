"""lhpc_csr_transpose and LHPC_PLAN_TRANSPOSE at the boundaries that need no
GPU: the symbol is declared, exported and mirrored; every argument error of
lhpc_csr_transpose is LHPC_ERR_INVALID_ARG (and nnz ≥ 2^32 LHPC_ERR_UNSUPPORTED)
before any device is touched; the flag's refusals are LHPC_ERR_UNSUPPORTED
before any device work; the Python wrappers reject wrong dtypes and sizes
before the C call; the C++ header surface compiles and links
(tests/cpp/test_transpose_api.cpp; run on the GPU by
tests/test_gpu_transpose.py).  The CPU oracle of the transposition lives here
(`transpose_oracle`) with tests of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests._support import ROOT

NAME = "lhpc_csr_transpose"
CPP_DIR = os.path.join(ROOT, "tests", "cpp")
CPP_BIN = os.path.join(CPP_DIR, "_build", "test_transpose_api")
TRANSPOSE = 1 << 11


def build_cpp():
    subprocess.run(["make", "-C", CPP_DIR, "-f", "transpose.mk"], check=True, capture_output=True)
    return CPP_BIN


def transpose_oracle(rp, col, val, n_cols):
    """(t_row_ptr, t_col_idx, t_val, perm) of include/lhpc.h lhpc_csr_transpose:
    a stable sort of the entry positions by column.  val may be None."""
    rp, col = np.asarray(rp), np.asarray(col)
    perm = np.argsort(col, kind="stable")
    row_of = np.repeat(np.arange(rp.size - 1, dtype=np.int32), np.diff(rp))
    t_col = row_of[perm].astype(np.int32)
    t_val = None if val is None else np.asarray(val)[perm]
    t_rp = np.searchsorted(col[perm], np.arange(n_cols + 1), side="left").astype(rp.dtype)  # #{p : col[p] < c}
    return t_rp, t_col, t_val, perm.astype(np.uint32)


# ------------------------------------------------------------------ the oracle itself
def _random_csr(n_rows, n_cols, seed, sort_rows):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 6, size=n_rows)
    rp = np.zeros(n_rows + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    cols = [rng.choice(n_cols, size=int(k), replace=False) for k in lens]
    if sort_rows:
        cols = [np.sort(c) for c in cols]
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    return rp, col, rng.uniform(-1, 1, col.size)


def test_oracle_transpose_twice_is_the_identity_on_sorted_rows():
    rp, col, val = _random_csr(37, 23, 1, sort_rows=True)
    t_rp, t_col, t_val, perm = transpose_oracle(rp, col, val, 23)
    assert t_rp[0] == 0 and t_rp[-1] == col.size and np.array_equal(np.sort(perm), np.arange(col.size))
    b_rp, b_col, b_val, _ = transpose_oracle(t_rp, t_col, t_val, 37)
    assert np.array_equal(b_rp, rp) and np.array_equal(b_col, col) and np.array_equal(b_val, val)
    dense = np.zeros((37, 23))
    dense[np.repeat(np.arange(37), np.diff(rp)), col] = val
    dense_t = np.zeros((23, 37))
    dense_t[np.repeat(np.arange(23), np.diff(t_rp)), t_col] = t_val
    assert np.array_equal(dense_t, dense.T)


def test_oracle_keeps_duplicates_in_input_order():
    rp = np.array([0, 3, 5], dtype=np.int64)
    col = np.array([1, 1, 0, 1, 1], dtype=np.int32)  # (0,1) twice, (1,1) twice
    val = np.array([10.0, 20.0, 30.0, 40.0, 50.0])
    t_rp, t_col, t_val, perm = transpose_oracle(rp, col, val, 3)
    assert t_rp.dtype == np.int64 and t_rp.tolist() == [0, 1, 5, 5]
    assert t_col.tolist() == [0, 0, 0, 1, 1] and t_val.tolist() == [30.0, 10.0, 20.0, 40.0, 50.0]
    assert perm.tolist() == [2, 0, 1, 3, 4]


def test_oracle_sorts_unsorted_rows():
    rp, col, val = _random_csr(41, 29, 2, sort_rows=False)
    t_rp, t_col, t_val, _ = transpose_oracle(rp, col, val, 29)
    for c in range(29):
        assert np.all(np.diff(t_col[t_rp[c]:t_rp[c + 1]]) > 0)  # distinct columns per row: strictly ascending
    b_rp, b_col, _, _ = transpose_oracle(t_rp, t_col, t_val, 41)
    assert np.array_equal(b_rp, rp)
    for r in range(41):
        assert np.array_equal(b_col[rp[r]:rp[r + 1]], np.sort(col[rp[r]:rp[r + 1]]))
    assert transpose_oracle(rp, col, None, 29)[2] is None


# ------------------------------------------------------------------ the symbol
def test_symbol_exported_and_mirrored(lhpc):
    from tests.test_abi import declared_functions
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "libhpc_amd", "_lib", "liblhpc.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert NAME in declared_functions(), f"{NAME} not declared in include/lhpc.h"
    assert NAME in lhpc.ABI_SYMBOLS and NAME in exported
    assert len(getattr(lhpc.lib, NAME).argtypes) == 14
    assert lhpc.PLAN_TRANSPOSE == TRANSPOSE and callable(lhpc.csr_transpose)
    hdr = open(os.path.join(ROOT, "include", "lhpc.h")).read()
    assert "LHPC_PLAN_TRANSPOSE = 1u << 11" in hdr and "#define LHPC_ABI_VERSION 1" in hdr


# ------------------------------------------------------------------ argument checks, no device
def _call(lhpc, **kw):
    a = dict(dtype=0, n_rows=2, n_cols=3, nnz=2, rp=np.array([0, 1, 2], np.int32), bits=32,
             col=np.array([0, 2], np.int32), val=np.ones(2, np.float32), t_rp=np.zeros(4, np.int32),
             t_col=np.zeros(2, np.int32), t_val=np.zeros(2, np.float32), perm=np.zeros(2, np.uint32), on_device=0)
    a.update(kw)
    p = lambda v: None if v is None else v.ctypes.data  # noqa: E731
    return lhpc.lib.lhpc_csr_transpose(a["dtype"], a["n_rows"], a["n_cols"], a["nnz"], p(a["rp"]), a["bits"],
                                       p(a["col"]), p(a["val"]), p(a["t_rp"]), p(a["t_col"]), p(a["t_val"]),
                                       p(a["perm"]), a["on_device"], None)


BAD_ARGS = {
    "dtype": dict(dtype=2), "dtype_negative": dict(dtype=-1), "bits16": dict(bits=16), "bits0": dict(bits=0),
    "n_rows_negative": dict(n_rows=-1), "n_cols_negative": dict(n_cols=-1), "nnz_negative": dict(nnz=-1),
    "n_rows_past_int32": dict(n_rows=2**31), "n_cols_past_int32": dict(n_cols=2**31),
    "nnz_past_int32_with_32_bit_offsets": dict(nnz=2**31),
    "null_row_ptr": dict(rp=None), "null_t_row_ptr": dict(t_rp=None), "null_col_idx": dict(col=None),
    "null_t_col_idx": dict(t_col=None), "val_without_t_val": dict(t_val=None), "t_val_without_val": dict(val=None),
}


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("bad", list(BAD_ARGS))
def test_invalid_arguments_without_a_device(lhpc, bad, on_device):
    assert _call(lhpc, on_device=on_device, **BAD_ARGS[bad]) == -1


def test_nnz_at_the_sort_limit_is_unsupported_without_a_device(lhpc):
    for on_device in (0, 1):
        assert _call(lhpc, nnz=2**32, bits=64, on_device=on_device) == -5
        assert _call(lhpc, nnz=2**32, bits=32, on_device=on_device) == -1  # the argument check comes first


# ------------------------------------------------------------------ flag refusals, no device work
def _plan_opts(lhpc, flags, n_devices=0, device_ids=None, n_splits=0, options=None):
    rp, col, val = np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 0], np.int32), np.ones(3, np.float32)
    h = C.c_void_p()
    ids = None if device_ids is None else (C.c_int * len(device_ids))(*device_ids)
    sp = np.array([1, 2], np.int64)
    o = None if options is None else C.byref(lhpc.Options(**options))
    st = lhpc.lib.lhpc_spmv_plan_create_opts(C.byref(h), 0, 3, 2, 3, rp.ctypes.data, 32, col.ctypes.data,
                                             val.ctypes.data, ids, n_devices, flags, n_splits,
                                             sp.ctypes.data if n_splits else None, o)
    return st, h


def test_transpose_refusals_before_any_device_work(lhpc):
    """n_splits > 0, n_devices > 1 and options.multi_force with the flag:
    LHPC_ERR_UNSUPPORTED, with device ordinals that do not exist (touching one
    would be a HIP error, a positive status)."""
    for kw in (dict(n_splits=2), dict(n_devices=2, device_ids=[97, 98]),
               dict(n_devices=1, device_ids=[97], options={"multi_force": 1}),
               dict(n_devices=2, device_ids=[97, 98], n_splits=2)):
        st, h = _plan_opts(lhpc, TRANSPOSE, **kw)
        assert st == -5 and not h.value, kw
        st, h = _plan_opts(lhpc, TRANSPOSE | lhpc.PLAN_DEVICE_INPUT, **kw)
        assert st == -5 and not h.value, kw
    # the create_split entry point goes the same way
    rp, col, val = np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 0], np.int32), np.ones(3, np.float32)
    h, sp = C.c_void_p(), np.array([1], np.int64)
    assert lhpc.lib.lhpc_spmv_plan_create_split(C.byref(h), 0, 3, 2, 3, rp.ctypes.data, 32, col.ctypes.data,
                                                val.ctypes.data, None, 0, TRANSPOSE, 1, sp.ctypes.data) == -5
    # the argument checks still come first
    assert _plan_opts(lhpc, TRANSPOSE, n_devices=-1)[0] == -1


def test_transpose_rows_past_int32_are_invalid(lhpc):
    """A's rows become the operator's columns, which are int32."""
    rp = np.zeros(1, np.int64)
    h = C.c_void_p()
    assert lhpc.lib.lhpc_spmv_plan_create(C.byref(h), 0, 2**31, 2, 0, rp.ctypes.data, 64, None, None, None, 0,
                                          TRANSPOSE) == -1
    assert lhpc.lib.lhpc_spmm_plan_create(C.byref(h), 0, 2**31, 2, 0, rp.ctypes.data, 64, None, None, -1,
                                          TRANSPOSE) == -1


def test_dist_plan_refuses_the_flag_before_any_device_work(lhpc):
    """lhpc_dist_spmv_plan_create*: the flag is refused after the null-pointer
    checks and before the communicator is read (a zeroed stand-in here)."""
    comm = (C.c_char * 4096)()
    rp, cuts = np.array([0, 1, 2], np.int32), np.array([0, 2], np.int64)
    col, val = np.array([0, 1], np.int32), np.ones(2, np.float32)
    h = C.c_void_p()
    args = (C.byref(h), C.addressof(comm), 0, 2, 2, 1, cuts.ctypes.data, rp.ctypes.data, 32, col.ctypes.data,
            val.ctypes.data, TRANSPOSE)
    assert lhpc.lib.lhpc_dist_spmv_plan_create_opts(*args, None) == -5 and not h.value
    assert lhpc.lib.lhpc_dist_spmv_plan_create(*args) == -5 and not h.value


# ------------------------------------------------------------------ the Python wrappers
class _NoCall:
    """Stands in for the C entry point: the wrapper must raise before calling it."""

    def __call__(self, *a):
        raise AssertionError("the C function was called")


def test_csr_transpose_wrapper_rejects_before_the_c_call(lhpc, monkeypatch):
    import torch
    monkeypatch.setattr(lhpc.lib, NAME, _NoCall())
    rp, col, val = np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), np.ones(2, np.float32)
    with pytest.raises(TypeError, match="row_ptr must be int32 or int64"):
        lhpc.csr_transpose(rp.astype(np.int16), col, val, 3)
    with pytest.raises(TypeError, match="col_idx int32"):
        lhpc.csr_transpose(rp, col.astype(np.int64), val, 3)
    with pytest.raises(TypeError, match="val must be float32 or float64"):
        lhpc.csr_transpose(rp, col, val.astype(np.float16), 3)
    with pytest.raises(TypeError, match="numpy arrays or CUDA tensors"):
        lhpc.csr_transpose([0, 1, 2], col, val, 3)
    with pytest.raises(TypeError, match="numpy arrays or CUDA tensors"):
        lhpc.csr_transpose(torch.from_numpy(rp), torch.from_numpy(col), torch.from_numpy(val), 3)  # CPU tensors
    with pytest.raises(ValueError, match="expected 2 values"):
        lhpc.csr_transpose(rp, col, np.ones(3, np.float32), 3)
    with pytest.raises(ValueError, match="one-dimensional"):
        lhpc.csr_transpose(rp, col.reshape(1, 2), None, 3)
    with pytest.raises(ValueError, match="one-dimensional"):
        lhpc.csr_transpose(np.zeros(0, np.int32), col, val, 3)
    with pytest.raises(ValueError, match="n_cols"):
        lhpc.csr_transpose(rp, col, val, -1)


@pytest.mark.parametrize("cls", ["SpMVPlan", "SpMMPlan"])
def test_plan_wrappers_take_the_keyword_and_reject_before_the_c_call(lhpc, monkeypatch, cls):
    """transpose=True reaches the C call as LHPC_PLAN_TRANSPOSE with A's shape,
    the plan's n_rows / n_cols are the operator's; wrong dtypes raise first."""
    seen = {}

    def fake(out, dtype, n_rows, n_cols, nnz, *rest):
        seen.update(n_rows=n_rows, n_cols=n_cols, flags=rest[-1])
        return -4  # LHPC_ERR_NO_DEVICE: the plan is not created

    name = "lhpc_spmv_plan_create" if cls == "SpMVPlan" else "lhpc_spmm_plan_create"
    monkeypatch.setattr(lhpc.lib, name, fake)
    rp, col, val = np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), np.ones(2, np.float32)
    with pytest.raises(lhpc.LhpcError):
        getattr(lhpc, cls)(rp, col, val, 3, transpose=True)
    assert seen == dict(n_rows=2, n_cols=3, flags=TRANSPOSE)
    monkeypatch.setattr(lhpc.lib, name, _NoCall())
    with pytest.raises(TypeError, match="row_ptr must be int32 or int64"):
        getattr(lhpc, cls)(rp.astype(np.int16), col, val, 3, transpose=True)
    with pytest.raises(TypeError, match="val must be float32 or float64"):
        getattr(lhpc, cls)(rp, col, val.astype(np.int32), 3, transpose=True)
    # a plan object without a device behind it: the operator's shape, values counted in A's order
    plan = getattr(lhpc, cls).__new__(getattr(lhpc, cls))
    plan.dtype, plan.np_dtype, plan.nnz, plan._h = lhpc.F32, np.dtype(np.float32), 2, C.c_void_p()
    monkeypatch.setattr(lhpc.lib, "lhpc_spmv_plan_set_values", _NoCall())
    monkeypatch.setattr(lhpc.lib, "lhpc_spmm_plan_set_values", _NoCall())
    with pytest.raises(ValueError, match="expected 2 values"):
        plan.set_values(np.zeros(3, np.float32))
    with pytest.raises(TypeError, match="expected dtype"):
        plan.set_values(np.zeros(2, np.float64))
    plan._h = None  # nothing to destroy


def test_cpp_header_compiles_and_links():
    """include/sparse/Transpose.hpp (both overloads) and the transposed plans
    of SpMV.hpp / SpMM.hpp, for float and double and 32- and 64-bit row
    offsets, in a stand-alone program built by tests/cpp/transpose.mk with
    -Wall -Wextra."""
    exe = build_cpp()
    assert os.path.exists(exe)
    out = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True, check=True).stdout
    assert NAME in out, f"the program does not call {NAME}"
