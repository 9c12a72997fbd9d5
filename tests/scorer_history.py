"""One `ld_scorer*` handle asked many things in a row: the configured calls of its entries (and of the `ld_gso*` objects that
share its workspace), what each must return, and the orders ("histories") in which tests/test_gpu_scorer_history.py puts them
to one handle.  A scorer keeps grow-only pose buffers (csrc/scorer.hpp: ws_partial_, ws_flags_, ws_counts_, ws_tested_,
ws_exact_, ws_poses_, ws_energies_), the block-major path a workspace whose regions are placed again at every call (by
bm_layout of the batch's shape: cap = min(n, pass size), one or two sets), the packed route its receptor images, refinement
and decomposition buffers of their own; nothing on the block-major path is memset.  Whatever a call does not write it inherits
from the call before, and what it inherits is plausible data.  So every (handle, entry) has a small PROBE and a large DECOY
that differ in everything that could be inherited -- other poses of other seeds, other sizes, rows wider than the pose, other
masks, steps, iteration counts, swarm and glowworm counts and seeds.

Nothing expected comes from the library: energies and pair counts are the oracle's (`energy_rows`, `energy_ex_row`), the
decomposition is test_gpu_decompose.restate, refinement is refine_reference.refine on the oracle's energies, a GSO is orc.GSO
stepped alongside.  Each expectation is computed once per configured call and read-only afterwards; handles that share a
complex share its calls and expectations.  This file introduces no tolerance: the measures are test_gpu_parity's.
tests/test_scorer_history_cpu.py proves on the oracle alone that the histories can fail.  No test functions here.

Handles (the route is fixed when a scorer is built, so each is built under its own environment):

    bm          small synthetic DFIRE complex, rigid                    block-major; fused and counting sequences; one set
    bm16        the same files, LIGHTDOCK_BM_CHUNK=16                   n <= 16 fused with cap = n; n > 16 in passes of 16, two sets
    bm-anm      the same files, 3 + 3 seeded modes                      the block-major ANM form, wild rows
    packed      the same files, LIGHTDOCK_DFIRE_KERNEL=packed           pose-major route, static receptor image
    packed-anm  3 + 3 modes, LIGHTDOCK_DFIRE_KERNEL=packed              one receptor image per pose in grow-only buffers
    allpairs    the same files, LIGHTDOCK_DFIRE_KERNEL=allpairs         pose_energy_pairs<DFIRE>, flags by memset
    dna         golden 1azp (DNA, 10 + 10 modes, restraints)            pose_energy_pairs<DNA>
    pydock      the same files and arguments, method pydock             pose_energy_pairs<PYDOCK>

The small complex is test_gpu_bm_launch_sequence's (150 receptor atoms: three tiles, the last ragged, 4 membrane beads, one
restraint; 100 ligand atoms, one restraint: 6 tile pairs), drawn from a seed of this file's.

What the binding cannot express: a pose list without its count (the list is the GSO's, inside the library), a stride for
ld_gso_create or for the scalar ld_scorer_energy.  The refusals of history 3 are a stride below the pose length and a null pose
buffer, for every entry that takes either."""
import collections
import ctypes as C
import os

import numpy as np

import refine_reference as rr
from conftest import case_kwargs, case_positions
from handle_history import leading  # noqa: F401 (the CPU test takes it from here)
from test_gpu_bm_launch_sequence import small_anm_kw, small_complex
from test_gpu_decompose import check_atoms, check_terms_exact, restate
from test_gpu_gso_shapes import _against_oracle
from test_gpu_parity import REL_TOL, bm_err, rel_err
from test_gpu_refine import same_bits

ENTRIES = ("energy_batch", "energy", "device_mask", "device_counts", "decompose", "refine", "gso", "zero_rows")
# handle -> (complex, environment around the scorer's construction, pair kernel it must report: kernel_info names the
# all-pairs kernel by the head of its instance's symbol, method 0 = DFIRE, 1 = DNA, whose pair loop PYDOCK shares)
HANDLES = collections.OrderedDict((
    ("bm", ("rigid", {}, "dfire_bm_pairs")),
    ("bm16", ("rigid", {"LIGHTDOCK_BM_CHUNK": "16"}, "dfire_bm_pairs")),
    ("bm-anm", ("anm", {}, "dfire_bm_pairs")),
    ("packed", ("rigid", {"LIGHTDOCK_DFIRE_KERNEL": "packed"}, "dfire_packed_pairs")),
    ("packed-anm", ("anm", {"LIGHTDOCK_DFIRE_KERNEL": "packed"}, "dfire_packed_pairs")),
    ("allpairs", ("rigid", {"LIGHTDOCK_DFIRE_KERNEL": "allpairs"}, "pose_energy_pairs<0")),
    ("dna", ("dna", {}, "pose_energy_pairs<1")),
    ("pydock", ("pydock", {}, "pose_energy_pairs<1")),
))
COMPLEXES = ("rigid", "anm", "dna", "pydock")
GRAPH_HANDLES = ("bm", "bm16", "dna")       # history 7: the handles named for it (Gso::run takes no graph path with receptor modes on DFIRE)
# the refusals an entry has (history 3)
REFUSALS = {"energy_batch": ("stride", "null"), "energy": ("null",), "device_mask": ("stride", "null"), "device_counts": ("stride", "null"),
            "decompose": ("stride", "null"), "refine": ("stride", "null"), "gso": ("null",), "zero_rows": ()}

COMPLEX_SEED, MODES_SEED = 52620, 52621
SENTINEL = -12345.0
COUNT_SENTINEL = 0xDEADBEEF
FAR_T = (500.0, -300.0, 200.0)
FLIP_BATCHES = (70, 5, 16, 17, 1, 0, 9, 70, 5)
OK, REFUSED = "ok", "refused"
Call = collections.namedtuple("Call", "name entry kind complex poses params")
Step = collections.namedtuple("Step", "call expect")
STATS = ("accepted", "halvings", "evaluations", "frozen")
SIDE_KEYS = ("sums", "pairs", "interface")


def measure_of(handle):
    """The handle's own measure of test_gpu_parity.py: bm_err where dfire_bm_pairs runs, rel_err elsewhere."""
    return bm_err if HANDLES[handle][2] == "dfire_bm_pairs" else rel_err


def unit(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


class World:
    """The complexes' files and oracles, the configured calls and their expected outputs."""

    def __init__(self, orc, table, directory):
        self.orc, self.table = orc, table
        rec, lig, kw = small_complex(np.random.default_rng(COMPLEX_SEED), table, str(directory))
        method, arec, alig, akw = case_kwargs("1azp", orc, table)
        self.build = {"rigid": ("dfire", rec, lig, kw), "anm": ("dfire", rec, lig, small_anm_kw(np.random.default_rng(MODES_SEED), kw)),
                      "dna": (method, arec, alig, akw), "pydock": ("pydock", arec, alig, akw)}
        assert method == "dna"
        self.cpu = {c: orc.Scorer(b[0], b[1], b[2], **b[3]) for c, b in self.build.items()}
        self.pose_len = {c: self.cpu[c].pose_len for c in COMPLEXES}
        assert self.pose_len == {"rigid": 7, "anm": 13, "dna": 27, "pydock": 27}
        self.golden = np.ascontiguousarray(case_positions("1azp", orc))
        self.threads = min(8, os.cpu_count() or 1)
        self._expected, self._molecules, self.tails = {}, {}, {}
        self.calls = {}
        for c in COMPLEXES:
            self.tails[c] = self._tail_poses(c)
            for entry in ENTRIES:
                for kind in ("probe", "decoy"):
                    self._add(self._configure(entry, kind, c))
            self._add(self._gso_call(c, "probe2", 1, 9, 4, 2))
            self._add(self._gso_call(c, "graph", 1, 9, 16, 3))
            # a refinement of more trial rows than any decoy's: it grows the workspace whatever ran before (history 6)
            self._add(self._made(c, "refine", "grow", self.decoy_rows(c, "refine", 30 if self.small(c) else 9, "grow"), iterations=2,
                                 steps=(1.5, 0.2, 0.8), max_halvings=1, slice_poses=0))
            for call in self._flips(c):
                self._add(call)

    # -- poses ------------------------------------------------------------------------------------------------------------

    def _rng(self, complex_, entry, kind, extra=0):
        return np.random.default_rng([COMPLEXES.index(complex_), ENTRIES.index(entry), sum(ord(ch) for ch in kind), extra])

    def small(self, complex_):
        return complex_ in ("rigid", "anm")

    def rows(self, rng, complex_, n, close, width=None):
        """n rows of `width` >= pose_len doubles.  close: near the receptor (clashes, flags and beads touched), non-unit
        quaternions, amplitudes of the order of 2; else spread out, unit quaternions, amplitudes of the order of 1.  Beyond
        pose_len: numbers no call may read."""
        L = self.pose_len[complex_]
        width = width or L
        p = np.zeros((n, width))
        if self.small(complex_):
            p[:, :3] = rng.uniform(-4.0, 4.0, (n, 3)) if close else rng.uniform(-22.0, 22.0, (n, 3))
            p[:, 3:7] = unit(rng, n) * (rng.uniform(0.5, 2.0, (n, 1)) if close else 1.0)
            p[:, 7:L] = rng.normal(size=(n, L - 7)) * (2.0 if close else 1.0)
        else:       # rows of the golden swarm, pulled towards the receptor or jittered away from each other
            pick = self.golden[rng.choice(len(self.golden), n, replace=n > len(self.golden))]
            p[:, :L] = pick
            p[:, :3] = pick[:, :3] * 0.85 + rng.normal(0.0, 0.3, (n, 3)) if close else pick[:, :3] * rng.uniform(1.0, 1.4, (n, 1)) + rng.normal(0.0, 1.5, (n, 3))
            p[:, 3:7] = unit(rng, n) * (rng.uniform(0.5, 2.0, (n, 1)) if close else 1.0)
            p[:, 7:L] = pick[:, 7:L] * (1.5 if close else 1.0) + rng.normal(0.0, 0.2, (n, L - 7))
        p[:, L:] = 1e3 * rng.normal(size=(n, width - L))
        return p

    def far_row(self, rng, complex_):
        row = self.rows(rng, complex_, 1, False)[0]
        row[:3] = FAR_T
        return row

    def tail_terms(self, complex_):
        """The indices into energy_ex_row's stats of the tail terms the complex has: 2 receptor restraint, 3 ligand restraint,
        4 membrane beads (1azp has none)."""
        return (2, 3, 4) if self.small(complex_) else (2, 3)

    def _tail_poses(self, complex_):
        """For every tail term of the complex a seeded pose that sets it, found on the oracle."""
        rng = np.random.default_rng([COMPLEXES.index(complex_), 777])
        found = {}
        for _ in range(40):
            cand = self.rows(rng, complex_, 16, True)
            cand[:, 3:7] = unit(rng, 16)
            for row in cand:
                stats = self.cpu[complex_].energy_ex_row(row)[1]
                for t in self.tail_terms(complex_):
                    if stats[t] > 0 and t not in found and not any(np.array_equal(row, f) for f in found.values()):
                        found[t] = row
            if len(found) == len(self.tail_terms(complex_)):
                return [found[t] for t in self.tail_terms(complex_)]
        raise AssertionError("no pose sets every tail term of %s: %s" % (complex_, sorted(found)))

    def probe_rows(self, complex_, entry, n):
        """At most 9 rows: the far pose and a pose for every tail term, then spread rows (the far pose and two tail poses
        where n is below that), in an order of the entry's own."""
        rng = self._rng(complex_, entry, "probe")
        head = [self.far_row(rng, complex_)] + list(self.tails[complex_])
        if n < len(head):
            return np.ascontiguousarray(np.stack([head[0], head[1], head[-1]][-n:]))
        rows = np.vstack([np.stack(head), self.rows(rng, complex_, n - len(head), False)]) if n > len(head) else np.stack(head)
        return np.ascontiguousarray(rows[rng.permutation(n)])

    def decoy_rows(self, complex_, entry, n, tag="decoy", extra=0):
        L = self.pose_len[complex_]
        rng = self._rng(complex_, entry, tag, extra)
        rows = self.rows(rng, complex_, n, True, L + 2)
        if L > 7:
            rows[min(4, n - 1), 7:L] *= 40.0        # one wild row (test_gpu_bm_launch_sequence.Small.anm_poses)
        return rows

    def swarm(self, complex_, rng, n, first):
        """A swarm of n glowworms close to each other and near the receptor, so that it moves: rows of exactly pose_len."""
        L = self.pose_len[complex_]
        p = np.zeros((n, L))
        if not self.small(complex_):      # around one row of the golden swarm
            base = self.golden[first % len(self.golden), :L]
            p[:] = base
            p[:, :3] += rng.normal(0.0, 1.5, (n, 3))
            q = base[3:7] + rng.normal(0.0, 0.1, (n, 4))
            p[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
            p[:, 7:] += rng.normal(0.0, 0.2, (n, L - 7))
            return p
        v = rng.normal(size=3)
        p[:, :3] = 11.0 * v / np.linalg.norm(v) + rng.normal(0.0, 1.5, (n, 3))
        p[:, 3:7] = unit(rng, n)
        p[:, 7:] = rng.normal(size=(n, L - 7))
        return p

    # -- the configured calls ---------------------------------------------------------------------------------------------

    def _add(self, call):
        assert call.name not in self.calls
        if call.poses is not None:
            call.poses.flags.writeable = False
        self.calls[call.name] = call

    def call(self, entry, kind, complex_):
        return self.calls["%s/%s/%s" % (complex_, entry, kind)]

    def of(self, handle, entry, kind):
        return self.call(entry, kind, HANDLES[handle][0])

    def _made(self, complex_, entry, kind, poses, **params):
        return Call("%s/%s/%s" % (complex_, entry, kind), entry, kind, complex_, poses, params)

    def _gso_call(self, complex_, kind, swarms, glowworms, steps, seed, still=None):
        rng = self._rng(complex_, "gso", kind, GSO_SEEDS[complex_].get(kind, 0))
        pos = np.stack([self.swarm(complex_, rng, glowworms, 30 * s + 7 * seed) for s in range(swarms)])
        if still is not None:       # a swarm whose glowworms share one pose: after the first step nothing moves, the list goes empty
            pos[still] = pos[still][2]
        return self._made(complex_, "gso", kind, pos, steps=steps, seeds=np.arange(swarms, dtype=np.uint64) * 1000 + 324324 + seed)

    def _configure(self, entry, kind, complex_):
        probe, small = kind == "probe", self.small(complex_)
        big = 70 if small else 24
        if entry == "energy_batch":
            if probe:
                return self._made(complex_, entry, kind, self.probe_rows(complex_, entry, 9))
            poses = self.decoy_rows(complex_, entry, big)
            # two degenerate rows (test_degenerate_poses_neither_hang_nor_poison_the_batch), beyond any probe's row count
            poses[11, 0] = np.nan
            poses[15, 3:7] = 0.0
            return self._made(complex_, entry, kind, poses, degenerate=(11, 15))
        if entry == "energy":
            rows = self.probe_rows(complex_, entry, 4) if probe else self.decoy_rows(complex_, entry, 1)[:, :self.pose_len[complex_]].copy()
            return self._made(complex_, entry, kind, np.ascontiguousarray(rows[-1:]))
        if entry in ("device_mask", "device_counts"):
            n = {"device_mask": 7, "device_counts": 5}[entry] if probe else big - 3 - (entry == "device_counts")
            poses = self.probe_rows(complex_, entry, n) if probe else self.decoy_rows(complex_, entry, n)
            active = np.ones(n, dtype=np.uint8)
            if probe:                     # a spread row; the far pose and the tail poses stay active
                special = [FAR_T] + [tuple(t[:3]) for t in self.tails[complex_]]
                active[[i for i in range(n) if tuple(poses[i, :3]) not in special][0]] = 0
            else:
                active[::3] = 0
            return self._made(complex_, entry, kind, poses, active=active, counts=entry == "device_counts")
        if entry == "decompose":
            return self._made(complex_, entry, kind, self.probe_rows(complex_, entry, 3) if probe else self.decoy_rows(complex_, entry, 12 if small else 5))
        if entry == "refine":
            # the seeds (the last argument) are chosen so that every decision gap of the restatement is at least MIN_GAP
            if probe:
                poses = self.rows(self._rng(complex_, entry, kind, REFINE_SEEDS[complex_][0]), complex_, 3, True)
                return self._made(complex_, entry, kind, poses, iterations=3 if small else 2, steps=(1.0, 0.1, 0.5), max_halvings=2, slice_poses=0)
            poses = self.decoy_rows(complex_, entry, 12 if small else 4, extra=REFINE_SEEDS[complex_][1])
            return self._made(complex_, entry, kind, poses, iterations=5 if small else 3, steps=(2.0, 0.3, 1.0), max_halvings=1, slice_poses=5 if small else 3)
        if entry == "gso":
            return self._gso_call(complex_, kind, 1, 9, 4, 1) if probe else self._gso_call(complex_, kind, 3, 24, 5, 5, still=1)
        assert entry == "zero_rows"
        return self._made(complex_, entry, kind, np.zeros((0, self.pose_len[complex_] + (0 if probe else 2))))

    def _flips(self, complex_):
        """History 4's calls: one entry asked again and again with other sizes and options, every call with rows of its own."""
        out = []
        for n in sorted(set(FLIP_BATCHES) - {0}):
            rows = self.decoy_rows(complex_, "energy_batch", n, "flip", n) if n > 9 else np.roll(self.probe_rows(complex_, "energy_batch", 9), n, axis=0)[:n].copy()
            out.append(self._made(complex_, "energy_batch", "flip-%d" % n, np.ascontiguousarray(rows)))
        for entry, n in (("device_counts", 9), ("device_mask", 65), ("device_counts", 65), ("device_mask", 9)):
            rows = self.decoy_rows(complex_, entry, n, "flip", n) if n > 9 else np.roll(self.probe_rows(complex_, entry, 9), 4, axis=0).copy()
            active = np.ones(n, dtype=np.uint8)
            active[1::4] = 0
            out.append(self._made(complex_, entry, "flip-%d" % n, rows, active=active, counts=entry == "device_counts"))
        base = self.call("refine", "probe", complex_)
        for tag, s in (("flip-sliced", 2), ("flip-whole", 0)):
            out.append(self._made(complex_, "refine", tag, base.poses, **dict(base.params, slice_poses=s)))
        return out

    def flip_history(self, handle):
        """4. inside an entry: energy_batch of n = 70, 5, 16, 17, 1, 0, 9, 70, 5; device_counts and device_mask alternating at
        n = 9 and 65; refine with slice_poses set and then unset; every probe in between."""
        c = HANDLES[handle][0]
        flips = [self.call("energy_batch", "flip-%d" % n, c) if n else self.call("zero_rows", "decoy", c) for n in FLIP_BATCHES]
        flips += [self.call(e, "flip-%d" % n, c) for e, n in (("device_counts", 9), ("device_mask", 65), ("device_counts", 65), ("device_mask", 9))]
        flips += [self.call("refine", "flip-sliced", c), self.call("refine", "flip-whole", c)]
        return [s for f in flips for s in [Step(f, OK)] + self.probes(handle)]

    # -- expectations -----------------------------------------------------------------------------------------------------

    def energies(self, complex_, rows):
        rows = np.ascontiguousarray(np.asarray(rows)[:, :self.pose_len[complex_]])
        if len(rows) == 0:
            return np.zeros(0)
        return self.cpu[complex_].energy_rows_mt(rows, self.threads) if len(rows) > 4 else self.cpu[complex_].energy_rows(rows)

    def molecules(self, complex_):
        """What test_gpu_decompose.restate takes: the oracle's model of each side, with its modes."""
        if complex_ not in self._molecules:
            kw, mols = self.build[complex_][3], []
            for side, tag in ((0, "rec"), (1, "lig")):
                mol = self.cpu[complex_].model(side)
                if kw.get("use_anm") and kw[tag + "_num_anm"] > 0:
                    mol["modes"] = np.asarray(kw[tag + "_nmodes"], dtype=np.float64).reshape(kw[tag + "_num_anm"], -1, 3)
                mols.append(mol)
            anm = (kw["rec_num_anm"], kw["lig_num_anm"]) if kw.get("use_anm") else (0, 0)
            self._molecules[complex_] = (mols[0], mols[1], anm)
        return self._molecules[complex_]

    def expected(self, call):
        """{output name: array} of a configured call; names that begin with "_" are what `held` needs beside them.  Computed
        once, read-only afterwards."""
        if call.name not in self._expected:
            out = self._compute(call)
            for v in out.values():
                if isinstance(v, np.ndarray):
                    v.flags.writeable = False
            self._expected[call.name] = out
        return self._expected[call.name]

    def _compute(self, call):
        c, p, poses, cpu = call.complex, call.params, call.poses, self.cpu[call.complex]
        L = self.pose_len[c]
        if call.entry in ("energy_batch", "energy", "zero_rows"):
            return {"energies": self.energies(c, poses)}
        if call.entry in ("device_mask", "device_counts"):
            on = p["active"] == 1
            out = {"energies": np.where(on, self.energies(c, poses), SENTINEL)}
            if p["counts"]:
                counts = np.array([cpu.energy_ex_row(row[:L])[1][5] for row in poses]).astype(np.int64)
                out["counts"] = np.where(on, counts, COUNT_SENTINEL).astype(np.uint32)
            return out
        if call.entry == "decompose":
            rec, lig, anm = self.molecules(c)
            want = [restate(self.orc, "dfire" if self.small(c) else "dna", rec, lig, self.table, row, *anm) for row in poses]
            out = {"_restated": want, "energy": np.array([w["terms"]["energy"] for w in want]),
                   "pairs": np.array([w["terms"]["pairs"] for w in want], dtype=np.uint32)}
            for key in ("rec", "lig"):
                for k in SIDE_KEYS:
                    out["%s/%s" % (key, k)] = np.stack([w[key][k] for w in want])
            return out
        if call.entry == "refine":
            r = rr.refine(self.orc.q_mul, lambda rows: self.energies(c, rows), poses, L, p["iterations"], p["max_halvings"], *p["steps"])
            out = {"poses": np.ascontiguousarray(r["poses"][:, :L]), "history": r["history"], "energy_before": r["before"], "energy_after": r["after"],
                   "_min_gap": r["min_gap"]}
            out.update({k: r["state"][k] for k in STATS})
            return out
        assert call.entry == "gso"
        refs = [self.orc.GSO(cpu, np.ascontiguousarray(poses[s]), seed=int(p["seeds"][s])) for s in range(len(poses))]
        steps = []
        for _ in range(p["steps"]):
            for ref in refs:
                ref.step()
            steps.append([ref.state() for ref in refs])
        out = {"_steps": steps, "num_evals": np.array([sum(ref.num_evals for ref in refs)], dtype=np.uint64), "steps_done": np.array([p["steps"]], dtype=np.uint32)}
        for s, state in enumerate(steps[-1]):
            out.update({"swarm%d/%s" % (s, k): v for k, v in state.items()})
        return out

    # -- the library's side -----------------------------------------------------------------------------------------------

    def make_scorer(self, pkg, handle, with_env):
        complex_, env, kernel = HANDLES[handle]
        method, rec, lig, kw = self.build[complex_]
        hip = with_env(env, lambda: pkg.Scorer.from_pdb(method, rec, lig, **kw))
        assert hip.kernel_info()["pair_kernel_name"] == kernel, (handle, hip.kernel_info()["pair_kernel_name"])
        assert hip.pose_len == self.pose_len[complex_]
        return hip

    def make_gso(self, pkg, hip, call):
        return pkg.GSO(hip, call.poses, seeds=call.params["seeds"])

    @staticmethod
    def gso_outputs(gso):
        out = {"num_evals": np.array([gso.num_evals], dtype=np.uint64), "steps_done": np.array([gso.steps_done], dtype=np.uint32)}
        for s in range(gso.n_swarms):
            out.update({"swarm%d/%s" % (s, k): v for k, v in gso.read(s).items()})
        return out

    def run(self, pkg, torch, hip, call):
        """The call on a scorer of its complex -> {output name: array}."""
        p, entry, poses = call.params, call.entry, call.poses
        L = hip.pose_len
        if entry in ("energy_batch", "zero_rows"):
            return {"energies": hip.energy_batch(poses)}
        if entry == "energy":
            row = poses[0]
            k = self.cpu[call.complex].anm_rec
            return {"energies": np.array([hip.energy(row[:3], row[3:7], row[7:7 + k], row[7 + k:L])])}
        if entry in ("device_mask", "device_counts"):
            n, dev = len(poses), torch.device("cuda:0")
            d_poses = torch.from_numpy(np.array(poses)).to(dev)
            d_out = torch.full((n,), SENTINEL, dtype=torch.float64, device=dev)
            d_active = torch.from_numpy(np.array(p["active"])).to(dev)
            d_cnt = torch.full((n,), COUNT_SENTINEL - (1 << 32), dtype=torch.int32, device=dev) if p["counts"] else None
            hip.set_stream(torch.cuda.current_stream().cuda_stream)
            try:
                hip.energy_batch_device(n, d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), d_active.data_ptr(), d_cnt.data_ptr() if p["counts"] else None)
                torch.cuda.synchronize()
            finally:
                hip.set_stream(0)
            out = {"energies": d_out.cpu().numpy()}
            if p["counts"]:
                out["counts"] = d_cnt.cpu().numpy().view(np.uint32)
            return out
        if entry == "decompose":
            got = hip.decompose(poses, atoms=True)
            out = {"_got": got, "energy": got["terms"]["energy"].copy(), "pairs": got["terms"]["pairs"].astype(np.uint32), "_terms": got["terms"]}
            for key in ("rec", "lig"):
                for k in SIDE_KEYS:
                    out["%s/%s" % (key, k)] = got[key][k]
            return out
        if entry == "refine":
            got = hip.refine(poses, p["iterations"], *p["steps"], max_halvings=p["max_halvings"], slice_poses=p["slice_poses"], history=True)
            st = got["stats"]
            out = {"poses": got["poses"], "history": got["history"], "energy_before": st["energy_before"].copy(), "energy_after": st["energy_after"].copy()}
            out.update({k: st[k].copy() for k in STATS})
            return out
        assert entry == "gso"
        gso = self.make_gso(pkg, hip, call)
        try:
            for _ in range(p["steps"]):
                gso.step()
            return self.gso_outputs(gso)
        finally:
            gso.close()

    def held(self, handle, hip, call, got):
        """The library's answer to a configured call against its expectation: energies under the handle's measure below
        REL_TOL, inactive rows at the sentinel, everything else to the bit or by the entry's own feature's check."""
        want, err = self.expected(call), measure_of(handle)
        p, entry = call.params, call.entry
        names = {k for k in want if not k.startswith("_")}
        assert {k for k in got if not k.startswith("_")} == names, call.name
        for k in names:
            assert got[k].shape == want[k].shape, (call.name, k, got[k].shape, want[k].shape)
        if entry in ("energy_batch", "energy", "zero_rows", "device_mask", "device_counts"):
            keep = np.ones(len(call.poses), dtype=bool)
            keep[list(p.get("degenerate", ()))] = False     # held as the degenerate-pose test holds them: the others unharmed
            on = keep & (p["active"] == 1 if "active" in p else True)
            if on.any():
                figure = err(got["energies"][on], want["energies"][on])
                print("%s on %s: %.2e" % (call.name, handle, figure))
                assert figure < REL_TOL, (call.name, handle, figure)
            assert np.all(got["energies"][keep & ~on] == SENTINEL), call.name
            if "counts" in want:
                assert np.array_equal(got["counts"], want["counts"]), call.name
        elif entry == "decompose":
            for i, w in enumerate(want["_restated"]):
                check_atoms(got["_got"], w, i, call.name)
                check_terms_exact(got["_terms"][i], w["terms"], (call.name, i))
        elif entry == "refine":
            for k in ("history",) + STATS:
                assert np.array_equal(got[k], want[k]), (call.name, k)
            assert same_bits(got["poses"], want["poses"]), call.name
            figures = (err(got["energy_before"], want["energy_before"]), err(got["energy_after"], want["energy_after"]))
            assert figures[0] < REL_TOL and figures[1] < REL_TOL, (call.name, figures)
        else:
            for s, state in enumerate(want["_steps"][-1]):
                _against_oracle(hip, {k: got["swarm%d/%s" % (s, k)] for k in state}, state, "%s swarm %d" % (call.name, s))
            assert np.array_equal(got["num_evals"], want["num_evals"]) and np.array_equal(got["steps_done"], want["steps_done"]), call.name

    def refuse(self, pkg, torch, hip, call, how):
        """A refused form of the call, straight through the C ABI: "stride" (below the pose length) or "null" (no pose buffer).
        -> (status, the outputs untouched)."""
        lib, p, entry, L = pkg.load_library(), call.params, call.entry, hip.pose_len
        poses = np.array(call.poses)
        n = len(poses) if entry != "gso" else poses.shape[1]
        stride = L - 1 if how == "stride" else poses.shape[-1]
        ptr = None if how == "null" else poses.ctypes.data_as(C.c_void_p)
        if entry == "energy_batch":
            out = np.full(n, SENTINEL)
            status = lib.ld_scorer_energy_batch(hip.handle, n, ptr, stride, out.ctypes.data_as(C.c_void_p))
            return status, np.all(out == SENTINEL)
        if entry == "energy":
            out = C.c_double(SENTINEL)
            amp = np.zeros(max(L - 7, 1))
            status = lib.ld_scorer_energy(hip.handle, None, poses[0, 3:7].copy().ctypes.data_as(C.c_void_p), amp.ctypes.data_as(C.c_void_p), amp.ctypes.data_as(C.c_void_p), C.byref(out))
            return status, out.value == SENTINEL
        if entry in ("device_mask", "device_counts"):
            dev = torch.device("cuda:0")
            d_poses = torch.from_numpy(poses).to(dev)
            d_out = torch.full((n,), SENTINEL, dtype=torch.float64, device=dev)
            d_active = torch.from_numpy(np.array(p["active"])).to(dev)
            d_cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
            status = lib.ld_scorer_energy_batch_device(hip.handle, n, None if how == "null" else C.c_void_p(d_poses.data_ptr()), stride, C.c_void_p(d_active.data_ptr()),
                                                       C.c_void_p(d_out.data_ptr()), C.c_void_p(d_cnt.data_ptr()) if p["counts"] else None)
            torch.cuda.synchronize()
            return status, bool((d_out == SENTINEL).all().item() and (d_cnt == -7).all().item())
        if entry == "decompose":
            terms = np.zeros(n, dtype=pkg.ENERGY_TERMS)
            terms.view(np.uint8)[:] = 3
            status = lib.ld_scorer_decompose(hip.handle, n, ptr, stride, terms.ctypes.data_as(C.c_void_p), None, None)
            return status, bool(np.all(terms.view(np.uint8) == 3))
        if entry == "refine":
            outs = (np.full((n, L), SENTINEL), np.zeros(n, dtype=pkg.REFINE_STATS), np.full((n, p["iterations"]), 77, dtype=np.int16))
            outs[1].view(np.uint8)[:] = 3
            opts = pkg._RefineOptions(p["iterations"], p["max_halvings"], p["steps"][0], p["steps"][1], p["steps"][2], p["slice_poses"], 0)
            status = lib.ld_scorer_refine(hip.handle, C.byref(opts), n, ptr, stride, *[a.ctypes.data_as(C.c_void_p) for a in outs])
            return status, bool(np.all(outs[0] == SENTINEL) and np.all(outs[1].view(np.uint8) == 3) and np.all(outs[2] == 77))
        assert entry == "gso" and how == "null"
        h = lib.ld_gso_create(hip.handle, poses.shape[0], poses.shape[1], None, None)
        return (-1 if not h and lib.ld_last_error() else 0), not h

    # -- the histories: lists of Step(call, OK or a refusal) --------------------------------------------------------------

    def probes(self, handle):
        return [Step(self.of(handle, e, "probe"), OK) for e in ENTRIES]

    def soak(self, handle):
        """1. every decoy once: every shared buffer ends larger than any probe needs."""
        return [Step(self.of(handle, e, "decoy"), OK) for e in ENTRIES]

    def pair_row(self, handle, x):
        """2. one row: decoy(X), then probe(Y), for every Y."""
        return [s for y in ENTRIES for s in (Step(self.of(handle, x, "decoy"), OK), Step(self.of(handle, y, "probe"), OK))]

    def refusals(self, handle, x):
        """3. before every probe, the refused forms of decoy(X)."""
        bad = [Step(self.of(handle, x, "decoy"), how) for how in REFUSALS[x]]
        return [s for y in ENTRIES for s in bad + [Step(self.of(handle, y, "probe"), OK)]]

    def growth(self, handle):
        """5. on a fresh handle (no soak): every probe, every decoy, every probe."""
        return self.probes(handle) + self.soak(handle) + self.probes(handle)

    def two_handles(self, a="bm", b="bm-anm"):
        """8. two handles turn by turn through history 2's first row; they share files and nothing else."""
        return [(h, s) for pair in zip(self.pair_row(a, ENTRIES[0]), self.pair_row(b, ENTRIES[0])) for h, s in zip((a, b), pair)]

    def between(self, handle):
        """6. what comes between the steps of a GSO that stays alive: every decoy (another GSO built, stepped and closed among
        them), then the refinement that grows the workspace."""
        return self.soak(handle) + [Step(self.call("refine", "grow", HANDLES[handle][0]), OK)]

    def quiet_decoys(self, handle):
        """7. decoys between two graph replays that do not grow the workspace: a smaller energy_batch, device_counts, decompose."""
        c = HANDLES[handle][0]
        return [Step(self.call("energy_batch", "flip-5", c), OK), Step(self.call("device_counts", "probe", c), OK), Step(self.call("decompose", "probe", c), OK)]


# seeds of the refine probe's and decoy's start poses per complex: tests/test_scorer_history_cpu.py holds every decision gap
# of the restatement at or above refine_cases.MIN_GAP with them
REFINE_SEEDS = {"rigid": (0, 0), "anm": (0, 0), "dna": (0, 0), "pydock": (0, 0)}
# seeds of the GSO calls' swarms per complex: with them every live swarm moves within its steps (held there too)
GSO_SEEDS = {"rigid": {"probe": 2, "probe2": 2, "decoy": 0, "graph": 0}, "anm": {"probe": 0, "probe2": 4, "decoy": 2, "graph": 0},
             "dna": {"probe": 2, "probe2": 1, "decoy": 0, "graph": 5}, "pydock": {"probe": 1, "probe2": 10, "decoy": 1, "graph": 0}}


