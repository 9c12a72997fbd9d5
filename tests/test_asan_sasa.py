"""Sanitizer run of the host side of the solvent-accessible surface path (ld_sasa_directions / ld_complex_sasa_radii /
ld_complex_sasa): every host source built by g++ with ASan + UBSan against tests/asan/hip_stub.cpp and
tests/asan/hip_stub_sasa.cpp (device memory = host memory; the sasa launch does its kernel's work in plain C++ from the
rule both sides share) and driven through the C ABI by the stand-alone tests/asan/sasa_check.cpp: two-atom cases whose
counts the rule pins, exclusions and radii, three 1czy poses (the first ranked model's sums pinned), more poses than
workspace slots, every NULL / non-NULL combination of the outputs, every refusal by status with the outputs untouched."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_asan import ENV, clean


@pytest.mark.timeout(900)
def test_sasa_host_side_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lightdock-rust_amd"), "-j8", "asan-sasa"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(ROOT, "lightdock-rust_amd", "build", "asan", "sasa_check")
    r = subprocess.run([exe, GOLDEN, str(tmp_path)], capture_output=True, text=True, env=ENV)
    out = r.stdout + r.stderr
    assert clean(out), out[-4000:]
    assert r.returncode == 0 and "sasa_check: 0 failures" in out, out[-3000:]
