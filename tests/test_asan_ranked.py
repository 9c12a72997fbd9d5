"""Sanitizer run of the host side of the ranked clustering (ld_complex_cluster_ranked): every host source
built by g++ with ASan + UBSan against tests/asan/hip_stub.cpp, tests/asan/hip_stub_assess.cpp and
tests/asan/hip_stub_ranked.cpp (device memory = host memory; the ranked launches do their kernels' work in plain C++ and
touch both ends of every buffer, so the host's round loop really runs and ends) and driven through the C ABI by
tests/asan/ranked_check.cpp: 1ppe poses under both measures against a sequential loop in the driver, n = 0, 1, 2, 63, 64,
65 and 150, ties in scoring, and every refusal by status with the outputs left as they were."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_asan import ENV, clean


@pytest.mark.timeout(900)
def test_ranked_host_side_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lightdock-rust_amd"), "-j8", "asan-ranked"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(ROOT, "lightdock-rust_amd", "build", "asan", "ranked_check")
    r = subprocess.run([exe, GOLDEN, str(tmp_path)], capture_output=True, text=True, env=ENV)
    out = r.stdout + r.stderr
    assert clean(out), out[-4000:]
    assert r.returncode == 0 and "ranked_check: 0 failures" in out, out[-3000:]
