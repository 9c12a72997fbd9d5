"""Sanitizer run of the host side of the small-angle scattering path (ld_complex_saxs_classes / ld_saxs_form_factors /
ld_saxs_sinc / ld_complex_distance_histogram / ld_saxs_debye / ld_complex_saxs / ld_saxs_fit): every host
source built by g++ with ASan + UBSan against tests/asan/hip_stub.cpp and tests/asan/hip_stub_saxs.cpp (device memory =
host memory; the saxs launches do their kernels' work in plain C++ from the rule both sides share) and driven through the
C ABI by the stand-alone tests/asan/saxs_check.cpp: the knife edges of a bin on two atoms, all 21 pair classes against a
count made in the driver, the Debye sum against the ordered loop on the library's own tables, three 1czy poses in one chunk
and in chunks of one, with and without a base row, every NULL / non-NULL combination of the outputs, every refusal by
status with the outputs untouched."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_asan import ENV, clean


@pytest.mark.timeout(900)
def test_saxs_host_side_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lightdock-rust_amd"), "-j8", "asan-saxs"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(ROOT, "lightdock-rust_amd", "build", "asan", "saxs_check")
    r = subprocess.run([exe, GOLDEN, str(tmp_path)], capture_output=True, text=True, env=ENV)
    out = r.stdout + r.stderr
    assert clean(out), out[-4000:]
    assert r.returncode == 0 and "saxs_check: 0 failures" in out, out[-3000:]
