"""Sanitizer run of the host side of the cross-link path (ld_complex_crosslinks): every host source built by
g++ with ASan + UBSan against tests/asan/hip_stub.cpp and tests/asan/hip_stub_xlink.cpp (device memory = host memory; the
xlink launches do their kernels' work in plain C++ from the rule both sides share) and driven through the C ABI by the
stand-alone tests/asan/xlink_check.cpp: one- and two-atom cases whose distances the rule pins, three 1czy poses, the links
reversed and repeated, more jobs than workspace slots, every NULL / non-NULL combination of the outputs, every refusal by
status with the outputs untouched."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_asan import ENV, clean


@pytest.mark.timeout(900)
def test_xlinks_host_side_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lightdock-rust_amd"), "-j8", "asan-xlinks"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(ROOT, "lightdock-rust_amd", "build", "asan", "xlink_check")
    r = subprocess.run([exe, GOLDEN, str(tmp_path)], capture_output=True, text=True, env=ENV)
    out = r.stdout + r.stderr
    assert clean(out), out[-4000:]
    assert r.returncode == 0 and "xlink_check: 0 failures" in out, out[-3000:]
