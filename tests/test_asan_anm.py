"""Sanitizer run of the host side of the normal-mode path (ld_anm_nodes / ld_anm_modes_xyz / ld_anm_modes):
every host source built by g++ with ASan + UBSan against tests/asan/hip_stub.cpp and tests/asan/hip_stub_anm.cpp (device
memory = host memory; the anm launches do their kernels' work in plain C++ with the rules both sides share) and driven
through the C ABI by the stand-alone tests/asan/anm_check.cpp: the 1czy peptide and the 2uuy ligand, whose modes the driver
checks for orthonormality, H v = lambda v, the sign rule, the extension to atoms and the amplitude rule; odd and even matrix
sizes; every refusal by status with the outputs untouched; NULL eigenvalues_out."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_asan import ENV, clean


@pytest.mark.timeout(900)
def test_anm_host_side_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lightdock-rust_amd"), "-j8", "asan-anm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(ROOT, "lightdock-rust_amd", "build", "asan", "anm_check")
    r = subprocess.run([exe, GOLDEN, str(tmp_path)], capture_output=True, text=True, env=ENV)
    out = r.stdout + r.stderr
    assert clean(out), out[-4000:]
    assert r.returncode == 0 and "anm_check: 0 failures" in out, out[-3000:]
