"""Sanitizer run of the host side of clustering by common contacts (ld_complex_pair_contacts / ld_fcc_common /
ld_fcc_cluster / ld_complex_cluster_fcc): every host source built by g++ with ASan + UBSan against
tests/asan/hip_stub.cpp and tests/asan/hip_stub_fcc.cpp (device memory = host memory; the fcc launches do their kernels' work
in plain C++ from the rule both sides share) and driven through the C ABI by the stand-alone tests/asan/fcc_check.cpp:
hand-made sets whose clusters the rule pins, three 1czy poses, every NULL / non-NULL combination of the outputs, every
refusal by status with the outputs untouched."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_asan import ENV, clean


@pytest.mark.timeout(900)
def test_fcc_host_side_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lightdock-rust_amd"), "-j8", "asan-fcc"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(ROOT, "lightdock-rust_amd", "build", "asan", "fcc_check")
    r = subprocess.run([exe, GOLDEN, str(tmp_path)], capture_output=True, text=True, env=ENV)
    out = r.stdout + r.stderr
    assert clean(out), out[-4000:]
    assert r.returncode == 0 and "fcc_check: 0 failures" in out, out[-3000:]
