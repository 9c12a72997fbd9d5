"""Sanitizer run of the host side of the model-quality path (ld_complex_set_reference / _assess): every host
source built by g++ with ASan + UBSan against tests/asan/hip_stub.cpp and tests/asan/hip_stub_assess.cpp (device memory =
host memory; the assess launches touch both ends of every buffer, walk the host-made lists whole and run the real f64
arithmetic after the sums) and driven through the C ABI by tests/asan/assess_check.cpp: matching, native pairs and used
atoms of 1ppe, more poses than a chunk and than the workspace slots, NULL outputs, every refusal by status, and the
eigensolver on half turns, a mirror image and degenerate sets."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_asan import ENV, clean


@pytest.mark.timeout(900)
def test_assess_host_side_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lightdock-rust_amd"), "-j8", "asan-assess"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(ROOT, "lightdock-rust_amd", "build", "asan", "assess_check")
    r = subprocess.run([exe, GOLDEN, str(tmp_path)], capture_output=True, text=True, env=ENV)
    out = r.stdout + r.stderr
    assert clean(out), out[-4000:]
    assert r.returncode == 0 and "assess_check: 0 failures" in out, out[-3000:]
