"""Sanitizer run of the host side of the energy decomposition (ld_scorer_decompose): every host source built
by g++ with ASan + UBSan against tests/asan/hip_stub.cpp and the analysis stubs (device memory = host memory) and
tests/asan/hip_stub_decompose.cpp, whose launches do their kernels' work in plain C++ and touch both ends of every buffer,
and driven through the C ABI by tests/asan/decompose_check.cpp: synthetic DFIRE and DNA complexes with and without ANM,
restraints and beads, n = 0, 1, 2 and slice + 1, NULL for each optional pointer, non-contiguous and empty groups and
LD_GROUP_NONE, every result bit for bit against a sequential loop in the driver, every refusal by status with the outputs
left as they were."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_asan import ENV, clean


@pytest.mark.timeout(900)
def test_decompose_host_side_under_asan_ubsan():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lightdock-rust_amd"), "-j8", "asan-decompose"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(ROOT, "lightdock-rust_amd", "build", "asan", "decompose_check")
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV)
    out = r.stdout + r.stderr
    assert clean(out), out[-4000:]
    assert r.returncode == 0 and "decompose_check: 0 failures" in out, out[-3000:]
