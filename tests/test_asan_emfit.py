"""Sanitizer run of the host side of the density-fit path (ld_density_* / ld_complex_density_fit /
ld_complex_simulate_density / ld_complex_density_chunk): every host source built by g++ with ASan + UBSan
against tests/asan/hip_stub.cpp and tests/asan/hip_stub_emfit.cpp (device memory = host memory; the emfit launches do
their kernels' work in plain C++ from the rule both sides share) and driven through the C ABI by the stand-alone
tests/asan/emfit_check.cpp: the quantisation, the table's plan, two atoms on two voxels worked out by hand, `outside`,
three 1czy poses in one chunk and in chunks of one with a rigid receptor and with zero-amplitude receptor modes, the sums
against the voxels, the scores' degenerate cases, every refusal by status with the outputs untouched."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_asan import ENV, clean


@pytest.mark.timeout(900)
def test_emfit_host_side_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lightdock-rust_amd"), "-j8", "asan-emfit"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(ROOT, "lightdock-rust_amd", "build", "asan", "emfit_check")
    r = subprocess.run([exe, GOLDEN, str(tmp_path)], capture_output=True, text=True, env=ENV)
    out = r.stdout + r.stderr
    assert clean(out), out[-4000:]
    assert r.returncode == 0 and "emfit_check: 0 failures" in out, out[-3000:]
