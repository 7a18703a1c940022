"""XTILE chunk records on the host (CPU, no GPU): tests/cpp/chunkrec_plan.cpp,
a stand-alone program with lhpc_plan.cpp compiled in under
-fsanitize=address,undefined (tests/cpp/chunkrec.mk), compares
xtile_chunk_records with a brute-force walk of the reduce kernel's own scan
and row decode — 3 and 256 tiles, one range and three ring ranges, a full
chunk, a last chunk of one nonzero, a row longer than a chunk, empty rows —
and puts xtile_policy's gating of the records to the C2 / C4 shapes and to
the shapes of the pinned small plans."""
import os
import subprocess

import pytest

from tests._support import ROOT

CPP_DIR = os.path.join(ROOT, "tests", "cpp")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_chunk_records_and_policy_under_sanitizers():
    r = subprocess.run(["make", "-C", CPP_DIR, "-f", "chunkrec.mk"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        pytest.fail(r.stdout[-2000:] + r.stderr[-2000:])
    r = subprocess.run([os.path.join(CPP_DIR, "_build", "asan", "chunkrec_plan")], capture_output=True, text=True,
                       timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ALL OK (chunk records)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_option_and_entry_point_are_mirrored(lhpc):
    """lhpc_options.xtile_chunkrec and lhpc_spmv_plan_chunkrec exist on both
    sides of the C ABI; a null plan is LHPC_ERR_INVALID_ARG before any device
    is touched."""
    import ctypes as C
    assert lhpc.Options(xtile_chunkrec=2).xtile_chunkrec == 2
    assert "lhpc_spmv_plan_chunkrec" in lhpc.ABI_SYMBOLS
    on = C.c_int(7)
    assert lhpc.lib.lhpc_spmv_plan_chunkrec(None, C.byref(on), None) == -1
