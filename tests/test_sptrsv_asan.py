"""Host sanitizer run of the triangular solve's analysis (CPU, no GPU):
libhpc_amd/csrc/lhpc_sptrsv_host.cpp — validation, levels, the sliced layout
and the launch schedule — compiled with -fsanitize=address,undefined into the
stand-alone program tests/cpp/asan_sptrsv.cpp (tests/cpp/sptrsv.mk `asan`),
which walks the test matrices of tests/test_sptrsv_api.py and the invalid
inputs that must come back as LHPC_ERR_BAD_CSR.  Run as tests/test_asan.py
runs its programs."""
import os
import subprocess

import pytest

from tests.test_asan import ENV, ROOT


def test_asan_sptrsv_analysis():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests/cpp"), "-f", "sptrsv.mk", "asan"],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        pytest.fail(r.stdout[-2000:] + r.stderr[-2000:])
    r = subprocess.run([os.path.join(ROOT, "tests/cpp/_build/asan/asan_sptrsv")], capture_output=True, text=True,
                       timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ALL OK (asan sptrsv)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
