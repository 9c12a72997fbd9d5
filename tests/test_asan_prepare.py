"""Sanitizer run of the host side of preparing a run (ld_swarm_diameter2 / ld_swarm_shell / ld_swarm_centres / ld_initial_poses /
ld_prepare_pdb): every host source built by g++ with ASan + UBSan against tests/asan/hip_stub.cpp and
tests/asan/hip_stub_prepare.cpp (device memory = host memory; the three launches do their kernels' work in plain C++ from the
predicates both sides share) and driven through the C ABI by the stand-alone tests/asan/prepare_check.cpp: the count-only call
and the filling one, a cap that is too small, every refusal by status with the outputs untouched, one atom, beads, the corners
of the coordinate range, a subset of 1czy, the pose rows and the cleaner.  The driver checks the answers against the rule as
it states it itself.  A program of its own: nothing is loaded into python."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_asan import ENV, clean


@pytest.mark.timeout(900)
def test_prepare_host_side_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lightdock-rust_amd"), "-j8", "asan-prepare"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(ROOT, "lightdock-rust_amd", "build", "asan", "prepare_check")
    r = subprocess.run([exe, GOLDEN, str(tmp_path)], capture_output=True, text=True, env=ENV)
    out = r.stdout + r.stderr
    assert clean(out), out[-4000:]
    assert r.returncode == 0 and "prepare_check: 0 failures" in out, out[-3000:]
