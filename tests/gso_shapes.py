"""Shapes at which the two GSO movement kernels (gso_step.hip: `gso_movement_phase`, one thread per glowworm, "single";
`gso_movement_phased`, 8 lanes per glowworm, "phased") take paths that the fixtures' swarms never reach: shares of a swarm
larger than a workgroup, ANM rows in the thread-per-glowworm kernel, mode counts other than 10 + 10, dynamic LDS at the
limit.  Shared by tests/test_gso_shapes_cpu.py (the oracle alone: the inputs reach what the table claims, far from any knife
edge) and tests/test_gpu_gso_shapes.py (the kernels against the oracle).  No test functions here.

The complex is "R": a seeded random rigid complex of 200 receptor and 130 ligand atoms in boxes of 28 and 18 angstroms,
scored by DFIRE with the synthetic table -- cheap for the oracle, so swarms of thousands of glowworms can be replayed.  Its
flexing variants carry random normal modes (normal * 0.4).

The launch arithmetic of gso.cpp (Gso::Gso: `parts`) and gso_step.hip (gso_step_is_phased, gso_kernel_lds_bytes,
launch_gso_step) is restated in `launch()`; every row of CASES spells out what it expects of it, and the CPU test asserts the
two equal: a change of the launch code makes the table fail instead of quietly losing the coverage.
"""
import os

import numpy as np

from test_gpu_parity import _random_molecule, _write_pdb

N_REC, N_LIG = 200, 130
COMPLEX_SEED = 20260
MODES_SEED = 977

LDS_LIMIT = 160 * 1024          # kGsoLdsLimit
MAX_GLOWWORMS = 4096            # Gso::Gso
PHASED_UP_TO = 65536            # glowworms in a launch up to which the launch's own choice is the phased kernel
LANES = 8                       # kGsoLanes
KEPT_UP_TO = 256                # swarms up to this size keep a bit per candidate for the roulette

K2_ALL = (None, "single", "phased")
STATE_KEYS = ("poses", "luciferin", "scoring", "vision_range", "n_neighbors", "target", "moved")


def _ceil_div(a, b):
    return -(-a // b)


def launch(n_swarms, n, k2):
    """What a step of `n_swarms` x `n` glowworms launches with LIGHTDOCK_GSO_K2 = k2 (None: unset)."""
    parts = min(_ceil_div(n, 64), max(1, _ceil_div(512, n_swarms)))
    share = _ceil_div(n, parts)
    phased = k2 == "phased" or (k2 != "single" and n_swarms * n <= PHASED_UP_TO)
    if phased and 6 * 8 * n > LDS_LIMIT:
        phased = False
    lds = (6 if phased else 4) * 8 * n
    threads = min(1024, _ceil_div(share * (LANES if phased else 1), 64) * 64)
    per_trip = threads // LANES if phased else threads
    shares = [min(n, (p + 1) * share) - p * share for p in range(parts)]
    # glowworms moved by each trip of the main loop, per workgroup of a swarm
    trips = [[min(per_trip, m - first) for first in range(0, m, per_trip)] for m in shares]
    return dict(parts=parts, share=share, shares=shares, kernel="phased" if phased else "single", threads=threads, lds=lds,
                trips=trips, second_walk=n > KEPT_UP_TO, words=_ceil_div(n, 64) if n <= KEPT_UP_TO else 0)


# id -> swarms S, glowworms N, modes (receptor, ligand) or None for the rigid complex, K2 settings, steps, swarm seed, and
# `expect`: per K2 setting what launch() must say -- the arithmetic of the issue's table, spelled out.
CASES = {
    # few modes; kept verdicts in three words (130 > 128).  parts = min(ceil(130/64) = 3, 512) = 3, share = ceil(130/3) = 44
    "A1": dict(S=1, N=130, modes=(2, 3), k2=K2_ALL, steps=12, seed=11,
               expect={None: dict(kernel="phased", parts=3, share=44, threads=384, lds=6240, trips=[[44], [44], [42]], words=3),
                       "single": dict(kernel="single", parts=3, share=44, threads=64, lds=4160, trips=[[44], [44], [42]], words=3),
                       "phased": dict(kernel="phased", parts=3, share=44, threads=384, lds=6240, words=3)}),
    # rigid ligand side; N > 256: the roulette walks the swarm a second time.  parts = min(5, 512) = 5, share = 60;
    # phased: 512 threads = 64 groups for 60 glowworms -- 4 idle groups share the wave votes of the second walk
    "A2": dict(S=1, N=300, modes=(10, 0), k2=K2_ALL, steps=12, seed=12,
               expect={None: dict(kernel="phased", parts=5, share=60, threads=512, lds=14400, second_walk=True, trips=[[60]] * 5),
                       "single": dict(kernel="single", parts=5, share=60, threads=64, lds=9600, second_walk=True),
                       "phased": dict(kernel="phased", threads=512, second_walk=True)}),
    # rigid receptor side
    "A3": dict(S=1, N=300, modes=(0, 10), k2=K2_ALL, steps=12, seed=13,
               expect={None: dict(kernel="phased", parts=5, share=60, second_walk=True), "single": dict(kernel="single"),
                       "phased": dict(kernel="phased")}),
    # pose_len 7 + 64 + 64 = 135, the admitted maximum: anm_step's delta[kMaxAnm] is full
    "A4": dict(S=1, N=130, modes=(64, 64), k2=K2_ALL, steps=12, seed=14,
               expect={None: dict(kernel="phased", parts=3, share=44, words=3), "single": dict(kernel="single", words=3),
                       "phased": dict(kernel="phased")}),
    # the same beyond 256
    "A5": dict(S=1, N=300, modes=(64, 64), k2=K2_ALL, steps=12, seed=15,
               expect={None: dict(kernel="phased", parts=5, share=60, second_walk=True),
                       "single": dict(kernel="single", second_walk=True), "phased": dict(kernel="phased")}),
    # 527 360 glowworms: single is the launch's own choice.  parts = min(17, ceil(512/512) = 1) = 1, share 1030, 1024 threads:
    # a second trip of 6 threads
    "B1": dict(S=512, N=1030, modes=None, k2=(None, "single"), steps=5, seed=100,
               expect={None: dict(kernel="single", parts=1, share=1030, threads=1024, lds=32960, trips=[[1024, 6]]),
                       "single": dict(kernel="single", parts=1, share=1030, threads=1024, lds=32960, trips=[[1024, 6]])}),
    # 537 600 glowworms.  parts = min(33, 2) = 2, share 1050: second trips of 26 threads (glowworms 1024..1049 and 2074..2099);
    # 4 * 8 * 2100 = 67 200 B of LDS, above the 64 KiB a kernel gets without asking
    "B2": dict(S=256, N=2100, modes=None, k2=(None, "single"), steps=5, seed=220,
               expect={None: dict(kernel="single", parts=2, share=1050, threads=1024, lds=67200, trips=[[1024, 26], [1024, 26]]),
                       "single": dict(kernel="single", parts=2, share=1050, threads=1024, lds=67200, trips=[[1024, 26], [1024, 26]])}),
    # 131 840 glowworms, phased forced.  parts = min(17, 4) = 4, share = ceil(1030/4) = 258: shares 258, 258, 258, 256; 1024 threads
    # = 128 glowworms a trip: trips 128 / 128 / 2 (and 128 / 128), with N > 256.  `single` is what it is compared with bit for bit.
    "B3": dict(S=128, N=1030, modes=None, k2=("phased", "single"), steps=5, seed=300,
               expect={"phased": dict(kernel="phased", parts=4, share=258, shares=[258, 258, 258, 256], threads=1024, lds=49440,
                                      trips=[[128, 128, 2]] * 3 + [[128, 128]], second_walk=True),
                       "single": dict(kernel="single", parts=4, share=258, threads=320, lds=32960)}),
    # phased at 48 * 3413 = 163 824 B of 163 840 B.  parts = min(54, 512) = 54, share = ceil(3413/54) = 64
    "C1": dict(S=1, N=3413, modes=None, k2=K2_ALL, steps=3, seed=21,
               expect={None: dict(kernel="phased", parts=54, share=64, threads=512, lds=163824),
                       "single": dict(kernel="single", lds=109216, threads=64), "phased": dict(kernel="phased", lds=163824)}),
    # 48 * 3414 = 163 872 B > 160 KiB: phased asked for (and the launch's own choice by size), single runs
    "C2": dict(S=1, N=3414, modes=None, k2=K2_ALL, steps=3, seed=22,
               expect={None: dict(kernel="single", parts=54, share=64, threads=64, lds=109248),
                       "single": dict(kernel="single", lds=109248), "phased": dict(kernel="single", lds=109248)}),
    # the largest swarm Gso admits: 4 * 8 * 4096 = 131 072 B in the thread-per-glowworm kernel.  parts = 64, share = 64
    "C3": dict(S=1, N=4096, modes=None, k2=K2_ALL, steps=3, seed=23,
               expect={None: dict(kernel="single", parts=64, share=64, threads=64, lds=131072),
                       "single": dict(kernel="single", lds=131072), "phased": dict(kernel="single", lds=131072)}),
}

# B3: the glowworms of the third trips of the three 258-shares
B3_THIRD_TRIP = (256, 257, 514, 515, 772, 773)


def sampled_swarms(case):
    s = CASES[case]["S"]
    return (0,) if s == 1 else (0, s // 2, s - 1)


class Shapes:
    """The complex R, its flexing variants and the cases' swarms; oracle scorers and oracle replays are made once."""

    def __init__(self, pkg, orc, table, directory):
        self.pkg, self.orc, self.table = pkg, orc, table
        rng = np.random.default_rng(COMPLEX_SEED)
        self.rec, self.lig = os.path.join(directory, "R_rec.pdb"), os.path.join(directory, "R_lig.pdb")
        self.rec_atoms = _random_molecule(rng, N_REC, 28.0, "A")
        self.lig_atoms = _random_molecule(rng, N_LIG, 18.0, "B")
        _write_pdb(self.rec, self.rec_atoms)
        _write_pdb(self.lig, self.lig_atoms)
        self._cpu, self._hip, self._replays = {}, {}, {}

    def scorer_kwargs(self, modes):
        kw = dict(potential=self.table)
        if modes is not None:
            k_rec, k_lig = modes
            rng = np.random.default_rng(MODES_SEED + 100 * k_rec + k_lig)
            kw.update(use_anm=True, rec_num_anm=k_rec, lig_num_anm=k_lig,
                      rec_nmodes=(rng.normal(size=(k_rec, N_REC, 3)) * 0.4).ravel() if k_rec else None,
                      lig_nmodes=(rng.normal(size=(k_lig, N_LIG, 3)) * 0.4).ravel() if k_lig else None)
        return kw

    def cpu(self, modes):
        if modes not in self._cpu:
            self._cpu[modes] = self.orc.Scorer("dfire", self.rec, self.lig, **self.scorer_kwargs(modes))
        return self._cpu[modes]

    def hip(self, modes):
        if modes not in self._hip:
            self._hip[modes] = self.pkg.Scorer.from_pdb("dfire", self.rec, self.lig, **self.scorer_kwargs(modes))
        return self._hip[modes]

    def swarms(self, case):
        """(positions (S, N, pose_len), seeds (S,) uint64): 16 distinct position sets cycled, every swarm its own seed, the
        (positions, seed) pair of swarm 1 again at S - 1."""
        c = CASES[case]
        extra = sum(c["modes"]) if c["modes"] else 0
        sets = [self.pkg.synth.swarm(c["N"], seed=c["seed"] + k, extra_cols=extra) for k in range(min(16, c["S"]))]
        positions = np.stack([sets[s % 16] for s in range(c["S"])])
        seeds = (np.arange(c["S"]) + 324324 + 1000 * c["seed"]).astype(np.uint64)
        if c["S"] > 1:
            positions[c["S"] - 1] = positions[1]
            seeds[c["S"] - 1] = seeds[1]
        return positions, seeds

    def replay(self, case):
        """{swarm: [state before the first step, state after step 1, ...]} of the oracle, for the sampled swarms.  The state
        before the first step is Glowworm::new's (luciferin 5, vision range 0.2)."""
        if case not in self._replays:
            c = CASES[case]
            positions, seeds = self.swarms(case)
            out = {}
            for s in sampled_swarms(case):
                ref = self.orc.GSO(self.cpu(c["modes"]), positions[s], seed=int(seeds[s]))
                states = [ref.state()]
                for _ in range(c["steps"]):
                    ref.step()
                    states.append(ref.state())
                states[-1]["num_evals"] = ref.num_evals
                out[s] = states
            self._replays[case] = out
        return self._replays[case]


_shared = None


def shapes(pkg, orc, table, directory):
    """One Shapes per test session: both test modules replay the oracle once."""
    global _shared
    if _shared is None:
        _shared = Shapes(pkg, orc, table, directory)
    return _shared
