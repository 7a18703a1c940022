"""Y = A·X (lhpc_spmm_*, libhpc_amd.SpMMPlan) checks that need no GPU: the
four entry points are exported and bound, every argument error is
LHPC_ERR_INVALID_ARG (a bad matrix LHPC_ERR_BAD_CSR) before any device is
touched, and the k_spmm_csr instantiations in the product library keep the
register budget DESIGN.md §4.2 states for them."""
import ctypes as C
import re

import numpy as np
import pytest

from tests.test_kernel_resources import BUNDLER, LIB, READELF, kernels

INVALID_ARG, BAD_CSR = -1, -2
SPMM_SYMBOLS = ("lhpc_spmm_plan_create", "lhpc_spmm", "lhpc_spmm_plan_info_get", "lhpc_spmm_plan_destroy")
# DESIGN.md §4.2 "register budget": every k_spmm_csr<T, I, P> within 64 VGPRs
# (8 waves per SIMD; LDS then sets 8 (fp32) / 6 (fp64) resident waves).  The
# issue's floor is 128 (4 waves per SIMD).
SPMM_VGPR_BUDGET = 64


def test_symbols_exported_and_bound(lhpc):
    for n in SPMM_SYMBOLS:
        assert n in lhpc.ABI_SYMBOLS
        fn = getattr(lhpc.lib, n)
        assert fn.argtypes is not None and fn.restype is C.c_int, n
    assert "SpMMPlan" in lhpc.__all__ and callable(lhpc.SpMMPlan)


def test_plan_info_mirror_matches_header(lhpc, tmp_path):
    """libhpc_amd.SpMMPlanInfo has lhpc_spmm_plan_info's size and field offsets."""
    import os
    import subprocess
    from tests._support import ROOT
    fields = [f[0] for f in lhpc.SpMMPlanInfo._fields_]
    src = tmp_path / "probe.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"lhpc.h\"\nint main(void){\n"
                   "printf(\"size %zu\\n\", sizeof(lhpc_spmm_plan_info));\n"
                   + "".join(f"printf(\"{n} %zu\\n\", offsetof(lhpc_spmm_plan_info, {n}));\n" for n in fields)
                   + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                   check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(lhpc.SpMMPlanInfo)
    for n in fields:
        assert int(got[n]) == getattr(lhpc.SpMMPlanInfo, n).offset, n


def _create(lhpc, **kw):
    args = dict(out=True, dtype=0, n_rows=2, n_cols=2, nnz=2, row_ptr=np.array([0, 1, 2], np.int32), bits=32,
                col=np.array([0, 1], np.int32), val=np.ones(2, np.float32), device=-1, flags=0)
    args.update(kw)
    h = C.c_void_p()
    st = lhpc.lib.lhpc_spmm_plan_create(
        C.byref(h) if args["out"] else None, args["dtype"], args["n_rows"], args["n_cols"], args["nnz"],
        args["row_ptr"].ctypes.data if args["row_ptr"] is not None else None, args["bits"],
        args["col"].ctypes.data if args["col"] is not None else None,
        args["val"].ctypes.data if args["val"] is not None else None, args["device"], args["flags"])
    return st, h


@pytest.mark.parametrize("bad", [dict(out=False), dict(dtype=7), dict(dtype=-1), dict(bits=16), dict(bits=0),
                                 dict(row_ptr=None), dict(col=None), dict(val=None), dict(n_rows=-1),
                                 dict(n_cols=-1), dict(nnz=-3), dict(device=-2)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_plan_create_invalid_args(lhpc, bad):
    st, h = _create(lhpc, **bad)
    assert st == INVALID_ARG and not h.value


@pytest.mark.parametrize("flag", ["PLAN_FORCE_ROWGROUP", "PLAN_FORCE_ADAPTIVE", "PLAN_FORCE_XSLICE", "PLAN_FORCE_XTILE",
                                  "PLAN_FORCE_SELL", "PLAN_FAST_PARTIALS", "PLAN_EXACT_PARTIALS"])
def test_plan_create_rejects_family_flags(lhpc, flag):
    """One kernel family, no partial sums: a FORCE_* or *_PARTIALS flag is an
    argument error, alone or beside the accepted flags, host or device input."""
    f = getattr(lhpc, flag)
    for extra in (0, lhpc.PLAN_VALIDATE, lhpc.PLAN_DEVICE_INPUT):
        st, h = _create(lhpc, flags=f | extra)
        assert st == INVALID_ARG and not h.value


@pytest.mark.parametrize("flags", [0, 1])
def test_plan_create_bad_csr_before_any_device(lhpc, flags):
    """A is always checked (LHPC_PLAN_VALIDATE is implied), on the host for
    host input: the kernel indexes X by col_idx."""
    for kw in (dict(row_ptr=np.array([0, 2, 1], np.int32)), dict(row_ptr=np.array([1, 1, 2], np.int32)),
               dict(col=np.array([0, 2], np.int32)), dict(col=np.array([-1, 0], np.int32)),
               dict(row_ptr=np.array([0, 2, 1], np.int64), bits=64)):
        st, h = _create(lhpc, flags=flags, **kw)
        assert st == BAD_CSR and not h.value


def test_plan_create_without_device_fails_loudly(lhpc):
    if lhpc.device_count() > 0:
        pytest.skip("a GPU is present")
    st, h = _create(lhpc)
    assert st == -4 and not h.value  # LHPC_ERR_NO_DEVICE: no CPU fallback
    with pytest.raises(lhpc.LhpcError):
        lhpc.SpMMPlan(np.array([0, 1], np.int32), np.array([0], np.int32), np.ones(1, np.float32), 1)


def test_null_plan_calls(lhpc):
    L = lhpc.lib
    x = np.ones(4, np.float32)
    assert L.lhpc_spmm(None, 1, x.ctypes.data, 1, x.ctypes.data, 1, 1, None) == INVALID_ARG
    assert L.lhpc_spmm_plan_info_get(None, C.byref(lhpc.SpMMPlanInfo())) == INVALID_ARG
    assert L.lhpc_spmm_plan_destroy(None) == L.lhpc_spmv_plan_destroy(None) == 0


@pytest.mark.parametrize("k,ldx,ldy", [(0, 4, 4), (-1, 4, 4), (3, 2, 4), (3, 4, 2), (3, -1, 4), (1, 0, 1), (1, 1, 0)])
def test_spmm_size_errors_come_before_the_plan_is_read(lhpc, k, ldx, ldy):
    """k < 1, ldx < k and ldy < k are LHPC_ERR_INVALID_ARG.  lhpc_spmm checks
    them before it reads the plan (and before any HIP call), so without a
    device — where no plan can exist — a zeroed stand-in for the handle is
    enough to reach them."""
    stand_in = C.create_string_buffer(4096)
    x = np.ones(64, np.float32)
    y = np.ones(64, np.float32)
    for on_device in (0, 1):
        assert lhpc.lib.lhpc_spmm(stand_in, k, x.ctypes.data, ldx, y.ctypes.data, ldy, on_device, None) == INVALID_ARG
    assert (y == 1).all()


def test_python_wrapper_argument_errors(lhpc):
    with pytest.raises(TypeError):
        lhpc.SpMMPlan(np.array([0, 1], np.int16), np.array([0], np.int32), np.ones(1, np.float32), 1)
    with pytest.raises(TypeError):
        lhpc.SpMMPlan(np.array([0, 1], np.int32), np.array([0], np.int32), np.ones(1, np.int32), 1)
    with pytest.raises(lhpc.LhpcError) as e:
        lhpc.SpMMPlan(np.array([0, 1], np.int32), np.array([0], np.int32), np.ones(1, np.float32), -5)
    assert e.value.status == INVALID_ARG
    with pytest.raises(lhpc.LhpcError) as e:
        lhpc.SpMMPlan(np.array([0, 1], np.int32), np.array([3], np.int32), np.ones(1, np.float32), 2)
    assert e.value.status == BAD_CSR


def test_block2d_takes_column_slices_and_rejects_other_strides(lhpc):
    """X / Y handling of SpMMPlan.__call__: the row stride is the leading
    dimension (a column slice of a wider row-major array, no copy); a
    non-unit inner stride, a wrong dtype or rank raise."""
    wide = np.arange(40, dtype=np.float32).reshape(5, 8)
    ptr, dev, rows, k, ld = lhpc._block2d(wide[:, 2:5], np.float32)
    assert (ptr, dev, rows, k, ld) == (wide.ctypes.data + 8, False, 5, 3, 8)
    assert lhpc._block2d(wide, np.float32)[2:] == (5, 8, 8)
    assert lhpc._block2d(wide[:, 3:4], np.float32)[2:] == (5, 1, 8)
    assert lhpc._block2d(wide[::2, 3:4], np.float32)[2:] == (3, 1, 16)  # k = 1: any inner stride
    assert lhpc._block2d(np.zeros((0, 4), np.float32), np.float32)[2:] == (0, 4, 4)
    for bad in (wide[:, ::2], wide.T, wide[::-1], np.asfortranarray(wide)):
        with pytest.raises(ValueError):
            lhpc._block2d(bad, np.float32)
    with pytest.raises(ValueError):
        lhpc._block2d(wide[0], np.float32)
    with pytest.raises(ValueError):
        lhpc._block2d(wide[:, :3], np.float32, k=4)
    with pytest.raises(TypeError):
        lhpc._block2d(wide.astype(np.float64), np.float32)
    with pytest.raises(TypeError):
        lhpc._block2d([[1.0]], np.float32)
    import torch
    t = torch.arange(40, dtype=torch.float64).reshape(5, 8)
    assert lhpc._block2d(t[:, 1:7], np.float64)[1:] == (False, 5, 6, 8)
    with pytest.raises(ValueError):
        lhpc._block2d(t[:, ::2], np.float64)
    with pytest.raises(TypeError):
        lhpc._block2d(t, np.float32)


@pytest.fixture(scope="module")
def spmm_kernels():
    import os
    if not os.path.exists(READELF) or not os.path.exists(BUNDLER) or not os.path.exists(LIB):
        pytest.skip("llvm-readelf / clang-offload-bundler or the built library not available")
    ks = {n: r for n, r in kernels().items() if "k_spmm_csr" in n}
    assert ks, "no k_spmm_csr kernel in the product library's code objects"
    return ks


def test_every_spmm_instantiation_is_in_the_code_object(spmm_kernels):
    """fp32/fp64 × int32/int64 row_ptr × panel widths 4, 8, 16, 32."""
    want = {f"k_spmm_csrI{t}{i}Li{p}EE" for t in "fd" for i in "il" for p in (4, 8, 16, 32)}
    got = {m.group(0) for n in spmm_kernels for m in [re.search(r"k_spmm_csrI[fd][il]Li\d+EE", n)] if m}
    assert got == want, sorted(want ^ got)
    assert len(spmm_kernels) == 16


def test_spmm_kernels_use_no_scratch_and_stay_in_budget(spmm_kernels):
    assert SPMM_VGPR_BUDGET <= 128  # 4 waves per SIMD: the floor for a gather-latency kernel
    for n, r in spmm_kernels.items():
        assert not r["vgpr_spill_count"] and not r["private_segment_fixed_size"], (n, r)
        assert not r["sgpr_spill_count"], (n, r)
        assert r["vgpr_count"] <= SPMM_VGPR_BUDGET, (n, r["vgpr_count"])
