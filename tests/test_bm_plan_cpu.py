"""How the block-major path cuts a launch's entries into (tile pair, part) pairs -- the arithmetic that dfire_bm_plan and every
workgroup of dfire_bm_census share (kernels/dfire_bm.hpp: bm_plan_entries, bm_part_size, bm_part_count, bm_census_plans) -- on
the host: a small C++ program built by g++ against the header prints what the functions give, and the rule is restated here.
No GPU: the kernels' use of it is tests/test_gpu_bm_launch_sequence.py."""
import os
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "lightdock-rust_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "kernels/dfire_bm.hpp"
// argv: waves part_cap count...   ->   P, then per tile pair "size parts first", then the number of pairs
int main(int argc, char **argv) {
    if (argc == 2) {   // the bound: tile pairs "n_rt n_lt plans" around it
        std::printf("%d %d %d\n", ld::kBmCensusTilePairs, ld::kBmPartEntries, ld::kBmAnmPartEntries);
        const size_t shapes[][2] = {{54, 52}, {256, 16}, {257, 16}, {4096, 1}, {4097, 1}, {1, 4096}, {64, 64}, {65, 64}, {141, 52}};
        for (auto &s : shapes) std::printf("%zu %zu %d\n", s[0], s[1], ld::bm_census_plans(s[0], s[1]) ? 1 : 0);
        return 0;
    }
    const uint32_t waves = (uint32_t)std::atol(argv[1]), part_cap = (uint32_t)std::atol(argv[2]);
    std::vector<uint32_t> count;
    for (int k = 3; k < argc; k++) count.push_back((uint32_t)std::atol(argv[k]));
    uint32_t total = 0;
    for (uint32_t c : count) total += c;
    const uint32_t P = ld::bm_plan_entries(total, waves, part_cap);
    std::printf("%u\n", P);
    uint32_t first = 0;
    for (uint32_t c : count) {
        std::printf("%u %u %u\n", ld::bm_part_size(c, P), ld::bm_part_count(c, P), first);
        first += ld::bm_part_count(c, P);
    }
    std::printf("%u\n", first);
    return 0;
}
"""


def build(tmp_path):
    src, exe = tmp_path / "bm_plan.cpp", tmp_path / "bm_plan"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-D__HIP_PLATFORM_AMD__",
                        "-I", os.path.join(ROCM, "include"), "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def plan(counts, waves, part_cap, part_entries=1792, factor=8):
    """DESIGN section 5, restated: P = total x 8 / waves rounded up to 64, within [64, part_cap]; a tile pair of n entries is cut into
    ceil(n / P) EQUAL parts of a multiple of 64 entries; the pairs are listed tile pair by tile pair."""
    total = int(sum(counts))
    cap = part_cap or part_entries
    P = min(max((total * factor // waves + 63) // 64 * 64, 64), cap)
    rows, first = [], 0
    for n in counts:
        parts = -(-n // P)
        size = (-(-n // parts) + 63) // 64 * 64 if parts else P
        k = -(-n // size) if n else 0
        rows.append((size, k, first))
        first += k
    return P, rows, first


def test_the_cut_into_parts(tmp_path):
    exe = build(tmp_path)
    rng = np.random.default_rng(5)
    cases = [
        (2048, 0, [0]), (2048, 0, [1]), (2048, 0, [64, 65, 0, 63]),
        (2048, 0, [200, 0, 199, 0, 0, 129]),                                   # the small test complex: P = 64, parts of 64
        (2048, 0, [int(v) for v in rng.integers(0, 8193, 300)]),               # a large launch: P at the cap
        (2048, 0, [int(v) for v in rng.integers(0, 300, 300)]),                # a late GSO step: P between the bounds
        (2048, 1024, [int(v) for v in rng.integers(0, 8193, 120)]),            # the ANM form's jobs
        (2048, 64, [1070, 5000, 0, 64, 1]),                                    # LIGHTDOCK_BM_PART_CAP=64
        (8 * 4, 0, [int(v) for v in rng.integers(0, 3000, 40)]),               # four CUs
        (2048, 0, [262144] * 16),                                              # a pass of 2^18 rows
    ]
    for waves, part_cap, counts in cases:
        r = subprocess.run([exe, str(waves), str(part_cap)] + [str(c) for c in counts], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.split("\n")
        P, rows, n_pairs = plan(counts, waves, part_cap)
        assert int(lines[0]) == P and P % 64 == 0
        got = [tuple(int(v) for v in line.split()) for line in lines[1:1 + len(counts)]]
        assert got == rows
        assert int(lines[1 + len(counts)]) == n_pairs
        for n, (size, k, _) in zip(counts, rows):
            assert size % 64 == 0 and size <= P and (k - 1) * size < n <= k * size if n else k == 0
        # the workspace has room for entries / 64 + tile pairs pairs (bm_layout: `parts`)
        assert n_pairs <= sum(counts) // 64 + len(counts)


def test_the_bound_of_the_census_plan(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe, "bound"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    bound, part_entries, anm_part_entries = (int(v) for v in lines[0].split())
    assert bound == 4096 == 4 * 1024 == 64 * 64        # four tile pairs a thread of the census' workgroup; two 64-way looks find a pair's tile pair
    assert part_entries == 1792 and anm_part_entries == 1024
    for line in lines[1:]:
        n_rt, n_lt, plans = (int(v) for v in line.split())
        assert plans == (1 if n_rt * n_lt <= bound else 0), line
    assert "54 52 1" in lines and "141 52 0" in lines   # 1k4c plans in the census; a 9 000-atom receptor against its ligand does not
