"""One `ld_complex*` handle asked many things in a row: the configured calls of all sixteen device entries, what each must
return, and the orders ("histories") in which tests/test_gpu_handle_history.py puts them to one handle.  The entries share
five grow-only device buffers and a handful of per-feature ones (csrc/complex.hpp); whatever a call does not write itself
it inherits from the call before, and what it inherits is plausible data, not garbage.  So every entry has a small PROBE and
a large DECOY with other poses, other scores, other parameters and every optional output; a probe that reads anything a
decoy (or a refused call) left behind returns something else than its expectation.

Nothing expected comes from the library: the posing, the thousandths and every rule are the restatements the suite already
has (ContactsRestated, bsas_edges.bsas on test_ranked_cpu's thousandths, fcc_reference, sasa_reference, ccs_reference,
xlink_reference, saxs_reference, emfit_reference, test_assess_cpu.AssessRestated, test_analysis_cpu.restated_pdb), each
computed once per configured call and cached in the World.  tests/test_handle_history_cpu.py proves on the restatements
alone that the histories can fail.  No test functions here; numpy and the standard library.

The complex is synthetic: 24 receptor and 9 ligand residues of N, CA, C, O, CB, SG, HA scattered in balls of 9 A and 5 A
whose centres are 13 A apart, one MMB bead (HETATM) a side, two seeded modes a side.  Two handles: "flex" (both sides' modes,
pose_len 11) and "rigid" (no receptor modes, pose_len 9: the receptor bitmaps of ccs, the base row of saxs, the base grid
of the density fit)."""
import collections
import os

import numpy as np

import bsas_edges as be
import ccs_reference as cr
import emfit_reference as er
import fcc_reference as fr
import sasa_reference as sr
import saxs_reference as sx
import xlink_reference as xr
from test_analysis_cpu import restated_pdb
from test_assess_cpu import FRAME_Q, FRAME_T, AssessRestated, moved, quaternion_matrix
from test_contacts_cpu import ContactsRestated
from test_ranked_cpu import RankedRestated

ENTRIES = ("coordinates", "cluster", "cluster_ranked", "contacts", "pair_contacts", "cluster_fcc", "sasa", "ccs", "crosslinks",
           "distance_histogram", "saxs", "density_fit", "simulate_density", "assess", "set_reference", "write_pdb")
HANDLES = ("flex", "rigid")
# entries that take one pose, or none: a decoy of theirs cannot ask for more poses than the probe
SINGLE = ("set_reference", "write_pdb")
# the coordinate bound of an entry, in A, as a translation that is beyond it (lightdock_hip.h); the others have none
FAR = {e: 1.1e6 for e in ENTRIES if e not in ("coordinates", "set_reference", "write_pdb")}
FAR["cluster"] = FAR["cluster_ranked"] = 2.2e6
ARGUMENT_REFUSALS = ("stride", "nan", "zero_quaternion")

N_REC_RES, N_LIG_RES = 24, 9
RESIDUE = (("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O"), ("CB", "C"), ("SG", "S"), ("HA", "H"))
REC_BALL, LIG_BALL, APART = 9.0, 5.0, 13.0
N_MODES = 2
XLINK_LDS_WORDS = 12288                   # kXlinkLdsWords (kernels/xlink.hpp)

OK, REFUSED = "ok", "refused"
Call = collections.namedtuple("Call", "name entry kind handle poses scores params")
Step = collections.namedtuple("Step", "call expect")


def xlink_bits_in_lds(max_length, cell):
    """xlink_bits_in_lds (kernels/xlink.hpp) of the two parameters in A."""
    M, h = int(round(1000.0 * max_length)), int(round(1000.0 * cell))
    side = 2 * (M // h) + 3 + (1 if M % h else 0)
    return (side ** 3 + 31) // 32 <= XLINK_LDS_WORDS


# ---- the complex --------------------------------------------------------------------------------------------------------------

def pdb_line(record, serial, name, resname, chain, seq, xyz, element):
    return "%-6s%5d  %-3s %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s\n" % (
        record, serial, name, resname, chain, seq, xyz[0], xyz[1], xyz[2], element)


def in_ball(rng, n, radius, centre):
    v = rng.normal(size=(n, 3))
    v *= (radius * rng.uniform(size=n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    return np.round(v + np.asarray(centre, dtype=np.float64), 3)


def side_text(rng, n_res, chain, radius, centre):
    xyz = in_ball(rng, n_res * len(RESIDUE) + 1, radius, centre)
    lines, serial = [], 0
    for r in range(n_res):
        for name, element in RESIDUE:
            lines.append(pdb_line("ATOM", serial + 1, name, "CYS", chain, r + 1, xyz[serial], element))
            serial += 1
    lines.append(pdb_line("HETATM", serial + 1, "BJ", "MMB", chain, n_res + 1, xyz[serial], "C"))
    return "".join(lines)


def random_poses(rng, shape, width, pose_len, spread=2.0):
    """Rows of `width` >= pose_len doubles: a translation within `spread` A, a random unit quaternion, amplitudes of the
    order of 1, and (beyond pose_len, where the stride is wider than the pose) numbers no call may read."""
    shape = tuple(shape)
    p = rng.normal(0.0, 1.0, shape + (width,))
    p[..., :3] = rng.uniform(-spread, spread, shape + (3,))
    p[..., 3:7] /= np.linalg.norm(p[..., 3:7], axis=-1, keepdims=True)
    p[..., pose_len:] = 1e3 * rng.normal(size=shape + (width - pose_len,))
    return p


def nudged(row, rng, by=0.02):
    """The same pose but for a few hundredths of an A: its twin in every clustering."""
    out = row.copy()
    out[:3] += rng.uniform(-by, by, 3)
    return out


Restatements = collections.namedtuple("Restatements", "em ccs xlink ranked")


class World:
    """The files of the synthetic complex in `directory`, the restatements of both handles, the configured calls and their
    expected outputs (computed on first use, then read-only)."""

    def __init__(self, directory):
        self.directory = str(directory)
        rng = np.random.default_rng(20240611)
        self.rec_pdb, self.lig_pdb = (os.path.join(self.directory, "history_%s.pdb" % s) for s in ("rec", "lig"))
        with open(self.rec_pdb, "w") as f:
            f.write(side_text(rng, N_REC_RES, "A", REC_BALL, (0.0, 0.0, 0.0)))
        with open(self.lig_pdb, "w") as f:
            f.write(side_text(rng, N_LIG_RES, "B", LIG_BALL, (APART, 0.0, 0.0)))
        self.n_rec, self.n_lig = N_REC_RES * len(RESIDUE) + 1, N_LIG_RES * len(RESIDUE) + 1
        self.rec_modes = rng.normal(0.0, 0.4, (N_MODES, self.n_rec, 3))
        self.lig_modes = rng.normal(0.0, 0.4, (N_MODES, self.n_lig, 3))
        self.pose_len = {"flex": 7 + 2 * N_MODES, "rigid": 7 + N_MODES}
        self.rs = {}
        for handle in HANDLES:
            args = (self.rec_pdb, self.lig_pdb, self.rec_modes if handle == "flex" else None, self.lig_modes)
            em = er.EmfitRestated(*args)
            self.rs[handle] = Restatements(em, cr.CcsRestated(*args), xr.XlinkRestated(*args), RankedRestated(em))
        # two maps of two shapes: rho (nz, ny, nx), origin and step (x, y, z) in thousandths, threshold
        self.maps = {"one": (rng.uniform(0.0, 1.0, (10, 11, 12)).astype(np.float32), (-6000, -12000, -10000), (3000, 3000, 3000), 0.3),
                     "two": (rng.uniform(0.0, 2.0, (7, 9, 8)).astype(np.float32), (-14000, -16000, -12000), (4000, 4000, 4000), 0.5)}
        self.references = self._write_references()
        self._assess_rs, self._expected, self._densities = {}, {}, {}
        self.calls = {}
        for handle in HANDLES:
            for entry in ENTRIES:
                for kind in ("probe", "decoy"):
                    self._add(self._configure(entry, kind, handle))
            for call in self._flips(handle):
                self._add(call)

    # -- files ------------------------------------------------------------------------------------------------------------

    def _write_references(self):
        """Reference A: the complex at a rigid pose near rest, in another frame.  B: at another pose, without two receptor
        residues and one ligand residue.  Rigid poses with every amplitude 0: the same files serve both handles."""
        em = self.rs["rigid"].em
        out = {}
        for name, t, q, dropped in (("A", (0.4, -0.3, 0.2), (1.0, 0.02, -0.01, 0.03), ((), ())),
                                    ("B", (-1.0, 0.8, 0.5), (0.95, -0.1, 0.2, 0.1), ((3, 17), (5,)))):
            row = np.array(list(t) + list(q) + [0.0] * N_MODES)
            lines = restated_pdb(em, self.rec_pdb, self.lig_pdb, row).splitlines()
            R = quaternion_matrix(FRAME_Q)
            paths = []
            for side, part, drop in (("rec", lines[:self.n_rec], dropped[0]), ("lig", lines[self.n_rec:], dropped[1])):
                kept = [l for l in moved(part, R, FRAME_T) if int(l[22:26]) - 1 not in drop]
                paths.append(os.path.join(self.directory, "history_ref%s_%s.pdb" % (name, side)))
                with open(paths[-1], "w") as f:
                    f.write("".join(l + "\n" for l in kept))
            out[name] = tuple(paths)
        return out

    def modes(self, handle):
        """Complex(rec_pdb, lig_pdb, *modes(handle))."""
        if handle == "flex":
            return self.rec_modes, N_MODES, self.lig_modes, N_MODES
        return None, 0, self.lig_modes, N_MODES

    def make_complex(self, pkg, handle):
        return pkg.Complex(self.rec_pdb, self.lig_pdb, *self.modes(handle))

    def density(self, pkg, which):
        """The pkg.Density of a map: one object for every handle of the session."""
        if which not in self._densities:
            rho, origin, step, threshold = self.maps[which]
            self._densities[which] = pkg.Density(rho, origin, step, threshold)
        return self._densities[which]

    def assess_restated(self, handle, reference, contact, interface):
        key = (handle, reference, contact, interface)
        if key not in self._assess_rs:
            rm, _, lm, _ = self.modes(handle)
            self._assess_rs[key] = AssessRestated(self.rec_pdb, self.lig_pdb, rm, lm, *self.references[reference],
                                                  contact_cutoff=contact, interface_cutoff=interface)
        return self._assess_rs[key]

    # -- the configured calls ---------------------------------------------------------------------------------------------

    def _add(self, call):
        assert call.name not in self.calls
        if call.poses is not None:
            call.poses.flags.writeable = False
        if call.scores is not None:
            call.scores.flags.writeable = False
        self.calls[call.name] = call

    def call(self, entry, kind, handle):
        return self.calls["%s/%s/%s" % (handle, entry, kind)]

    def _rng(self, *key):
        return np.random.default_rng([ENTRIES.index(key[0]), HANDLES.index(key[2]), sum(ord(c) for c in key[1])] + list(key[3:]))

    def _poses(self, entry, kind, handle, n, extra=0):
        """n seeded rows; a decoy's rows are two doubles wider than the pose (stride > pose_len)."""
        L = self.pose_len[handle]
        return random_poses(self._rng(entry, kind, handle, extra), (n,), L + (2 if kind == "decoy" else 0), L)

    def _configure(self, entry, kind, handle):
        probe = kind == "probe"
        L = self.pose_len[handle]
        rng = self._rng(entry, kind, handle, 99)
        n = {"probe": 2, "decoy": 24}[kind]
        scores, params = None, {}
        if entry == "cluster":
            if probe:             # one swarm of two pairs of twins: every row and every score decides something
                rows = self._poses(entry, kind, handle, 2)
                poses = np.stack([rows[0], nudged(rows[0], rng), rows[1], nudged(rows[1], rng)])[None]
                scores = np.array([[1.0, 3.0, 2.0, 4.0]])
            else:                 # 6 swarms x 8 glowworms, glowworm g + 4 the twin of glowworm g
                poses = random_poses(rng, (6, 8), L + 2, L)
                for s in range(6):
                    for g in range(4):
                        poses[s, g + 4] = nudged(poses[s, g], rng)
                scores = np.tile(np.array([10.0, 0.0, 20.0, 0.5, 7.0, 6.0, 9.0, 8.0]), (6, 1)) + rng.uniform(0.0, 0.1, (6, 8))
            params = {"cutoff": 1.0 if probe else 1.5}
        elif entry in ("cluster_ranked", "cluster_fcc"):
            if probe:             # two pairs of twins
                rows = self._poses(entry, kind, handle, 2)
                poses = np.stack([rows[0], nudged(rows[0], rng), rows[1], nudged(rows[1], rng)])
                scores = np.array([1.0, 3.0, 2.0, 4.0])
            else:
                poses = self._poses(entry, kind, handle, 32)
                for i in range(1, 32, 4):
                    poses[i] = nudged(poses[i - 1], rng)
                scores = np.concatenate([[10.0, 0.0, 20.0, 0.5], rng.uniform(0.0, 30.0, 28)])
            if entry == "cluster_ranked":
                # the ligand-only walk is the rigid handle's probe and the flex handle's decoy
                params = {"cutoff": 1.0 if probe else 1.5, "atoms": "ligand" if probe == (handle == "rigid") else "complex"}
            else:
                params = {"cutoff": 5.0, "threshold": 0.6, "min_size": 1} if probe else {"cutoff": 6.0, "threshold": 0.4, "min_size": 2}
        elif entry == "crosslinks":
            # anchors: receptor SG of residues 2 and 11, ligand SG of residues 1 and 6, a ligand CA, a receptor N
            a, b, c, d, e, g = 2 * 7 + 5, 11 * 7 + 5, self.n_rec + 7 + 5, self.n_rec + 6 * 7 + 5, self.n_rec + 3 * 7 + 1, 20 * 7
            if probe:             # two sources (a, b); its bits fit LDS
                poses = self._poses(entry, kind, handle, 1)
                params = {"links": np.array([[a, c], [a, d], [b, e], [b, g]], dtype=np.uint32), "probe": 0.0, "cell": 1.0, "reach": 3.0,
                          "max_length": 20.0, "paths": True}
            else:                 # one source (c) of five links; cell 0.5 and max_length 24 (19 on the rigid handle: half the nodes
                                  # for the restatement to walk): the bits of the box do not fit LDS and live in the slot.  Eight
                                  # poses, two of them distinct: the restatement walks a box of 10^6 nodes once per distinct pose
                poses = self._poses(entry, kind, handle, 8)
                poses[2:] = poses[np.arange(2, 8) % 2]
                params = {"links": np.array([[c, a], [c, b], [c, g], [c, e], [c, d]], dtype=np.uint32), "probe": 0.3, "cell": 0.5, "reach": 2.5,
                          "max_length": 24.0 if handle == "flex" else 19.0, "paths": True}
        elif entry == "assess":
            poses = self._poses(entry, kind, handle, n)
            if probe:             # the first pose is the reference's own but for a nudge
                poses[0, :7] = [0.4, -0.3, 0.2, 1.0, 0.02, -0.01, 0.03]
                poses[0, 7:L] = 0.0
                poses[0, 0] += 0.05
            params = {"reference": "A", "contact": 5.0, "interface": 10.0} if probe else {"reference": "B", "contact": 6.0, "interface": 12.0}
        elif entry == "set_reference":
            poses = None
            params = {"reference": "A", "contact": 5.0, "interface": 10.0} if probe else {"reference": "B", "contact": 6.0, "interface": 12.0}
        elif entry == "write_pdb":
            poses = self._poses(entry, "probe", handle, 1, extra=0 if probe else 1)        # one pose of exactly pose_len
        else:
            poses = self._poses(entry, kind, handle, n)
            params = {"coordinates": {},
                      "contacts": {"cutoff": 3.5 if probe else 7.5},
                      "pair_contacts": {"cutoff": 5.0 if probe else 6.5},
                      "sasa": {"probe": 1.4, "atoms": False} if probe else {"probe": 1.0, "atoms": True},
                      # the rigid form's bitmaps exist for what == 2 only: the rigid handle's decoy leaves them behind, laid
                      # out for a finer cell; the flex handle's decoy asks for another selection
                      "ccs": {"what": 2, "probe": 1.0, "cell": 0.5, "views": False} if probe else
                             {"what": 2 if handle == "rigid" else 1, "probe": 1.5, "cell": 0.3, "views": True},
                      "distance_histogram": {"width": 0.5, "bins": 128} if probe else {"width": 0.25, "bins": 1024},
                      "saxs": {"width": 0.5, "bins": 128, "q": np.array([0.0, 0.05, 0.2, 0.5]), "counts": False} if probe else
                              {"width": 0.3, "bins": 512, "q": np.linspace(0.01, 0.9, 9), "counts": True},
                      "density_fit": {"map": "one", "sigma": 2000} if probe else {"map": "two", "sigma": 3000},
                      "simulate_density": {"map": "one", "sigma": 2000} if probe else {"map": "two", "sigma": 3000}}[entry]
        return Call("%s/%s/%s" % (handle, entry, kind), entry, kind, handle, poses, scores, params)

    def _flips(self, handle):
        """History 4's calls: one entry asked again and again with other options and other n."""
        def made(entry, tag, n, **params):
            base = dict(self.call(entry, "probe", handle).params)
            base.update(params)
            poses = None if entry == "set_reference" else self._poses(entry, tag, handle, n)
            return Call("%s/%s/%s" % (handle, entry, tag), entry, tag, handle, poses, None, base)

        out = [made("sasa", "flip-on3", 3, atoms=True), made("sasa", "flip-off2", 2, atoms=False), made("sasa", "flip-on1", 1, atoms=True)]
        out += [made("ccs", "flip-%d-%s" % (k, what), 2, what=what, cell=cell, views=bool(k % 2))
                for k, (what, cell) in enumerate(((2, 0.5), (0, 0.5), (1, 2.0), (2, 2.0), (2, 0.5)))]
        links = self.call("crosslinks", "probe", handle).params["links"]
        out += [made("crosslinks", "flip-straight", 2, paths=False),
                made("crosslinks", "flip-reversed", 1, links=links[:, ::-1].copy()),
                made("crosslinks", "flip-regrouped", 1, links=np.array([links[0], links[2], [links[0][0], links[3][1]]], dtype=np.uint32))]
        for entry in ("distance_histogram", "saxs"):
            out += [made(entry, "flip-1024", 3, width=0.5, bins=1024, chunk=1), made(entry, "flip-64", 2, width=1.0, bins=64, chunk=0),
                    made(entry, "flip-1024-whole", 3, width=0.5, bins=1024, chunk=0), made(entry, "flip-64-by-one", 2, width=1.0, bins=64, chunk=1)]
        for k, (entry, which, chunk) in enumerate((("density_fit", "one", 1), ("simulate_density", "two", 0), ("density_fit", "two", 0),
                                                   ("simulate_density", "one", 1), ("density_fit", "one", 0))):
            out.append(made(entry, "flip-%d" % k, 3 - k % 2, map=which, chunk=chunk, sigma=2000 + 500 * (k % 2)))
        for k, which in enumerate("ABA"):
            cut = {"A": (5.0, 10.0), "B": (6.0, 12.0)}[which]
            out += [made("set_reference", "flip-%d" % k, 0, reference=which, contact=cut[0], interface=cut[1]),
                    made("assess", "flip-%d" % k, 2 + k, reference=which, contact=cut[0], interface=cut[1])]
        return out

    def flips(self, handle):
        return [c for c in self.calls.values() if c.handle == handle and c.kind.startswith("flip")]

    def refused(self, call, how):
        """The call with its last pose made unacceptable: "far" (beyond the entry's coordinate bound), "nan", "zero_quaternion",
        or every row cut below the pose length ("stride").  None where the entry has no such refusal."""
        if call.poses is None or (how == "far" and call.entry not in FAR) or (how == "stride" and call.entry == "write_pdb"):
            return None
        poses = call.poses.copy()
        last = poses.reshape(-1, poses.shape[-1])[-1]
        if how == "far":
            last[0] = FAR[call.entry]
        elif how == "nan":
            last[5] = np.nan
        elif how == "zero_quaternion":
            last[3:7] = 0.0
        else:
            assert how == "stride"
            poses = np.ascontiguousarray(poses[..., :self.pose_len[call.handle] - 1])
        return Call(call.name + "/" + how, call.entry, call.kind, call.handle, poses, call.scores, call.params)

    def refused_reference(self, handle):
        """A set_reference the library refuses: no native pair within a thousandth of an A."""
        p = dict(self.call("set_reference", "decoy", handle).params, contact=0.001)
        return Call("%s/set_reference/refused" % handle, "set_reference", "refused", handle, None, None, p)

    # -- expectations -----------------------------------------------------------------------------------------------------

    def expected(self, call):
        """{output name: array} of a configured call, by the restatements; "_measures" and "_rs" (assess) are what
        test_gpu_assess.assert_within_bounds takes.  Computed once, read-only afterwards."""
        if call.name not in self._expected:
            out = self._compute(call)
            for k, v in out.items():
                if isinstance(v, np.ndarray):
                    v.flags.writeable = False
            self._expected[call.name] = out
        return self._expected[call.name]

    def _compute(self, call):
        rs, p, entry = self.rs[call.handle], call.params, call.entry
        poses = call.poses
        if entry == "coordinates":
            return {"xyz": np.stack([rs.em.pose(row) for row in poses])}
        if entry in ("cluster", "cluster_ranked"):
            swarms = poses if entry == "cluster" else poses[None]
            scores = call.scores if entry == "cluster" else call.scores[None]
            atoms = p.get("atoms", "complex")
            n_atoms = len(rs.ranked.atoms[atoms])
            out = {"cluster_of": np.zeros(scores.shape, dtype=np.int32), "representatives": np.full(scores.shape, -1, dtype=np.int32),
                   "n_clusters": np.zeros(len(scores), dtype=np.uint32)}
            for s in range(len(swarms)):
                cluster_of, reps, ties = be.bsas(rs.ranked.thousandths(swarms[s], atoms), n_atoms, scores[s], p["cutoff"])
                assert ties == 0          # off every knife edge: the integer rule and the rounded one agree
                out["cluster_of"][s], out["representatives"][s, :len(reps)], out["n_clusters"][s] = cluster_of, reps, len(reps)
            return out
        if entry == "contacts":
            rec, lig = ContactsRestated.batch(rs.em, poses, p["cutoff"])      # EmfitRestated.batch is the histogram's
            return {"rec": rec, "lig": lig}
        if entry == "pair_contacts":
            offsets, keys = fr.pair_sets(rs.em, poses, p["cutoff"])
            return {"offsets": offsets, "keys": keys}
        if entry == "cluster_fcc":
            offsets, keys = fr.pair_sets(rs.em, poses, p["cutoff"])
            out = fr.cluster(offsets, keys, call.scores, p["threshold"], p["min_size"])
            out["n_clusters"] = np.array([out["n_clusters"]], dtype=np.int64)
            return out
        if entry == "sasa":
            sums, free, bound = sr.SasaRestated.batch(rs.xlink, poses, p["probe"])      # XlinkRestated is a SasaRestated
            return {"sums": sums, "free": free, "bound": bound} if p["atoms"] else {"sums": sums}
        if entry == "ccs":
            counts, sums = rs.ccs.batch(poses, p["what"], p["probe"], p["cell"])
            return {"sums": sums, "counts": counts} if p["views"] else {"sums": sums}
        if entry == "crosslinks":
            args = (p["probe"], p["cell"], p["reach"], p["max_length"])
            if p["paths"]:
                rows, where = np.unique(poses, axis=0, return_inverse=True)        # each distinct pose once
                straight2, path = rs.xlink.batch(rows, p["links"], *args)
                return {"straight2": straight2[where.ravel()], "path": path[where.ravel()]}
            got = [rs.xlink.crosslinks(row, p["links"], *args, paths=False)[0] for row in poses]
            return {"straight2": np.array(got, dtype=np.uint64).reshape(len(poses), len(p["links"]))}
        if entry in ("distance_histogram", "saxs"):
            w = int(round(1000.0 * p["width"]))
            counts = rs.em.batch(poses, w, p["bins"])
            if entry == "distance_histogram":
                return {"counts": counts}
            f, s = sx.form_factors(p["q"]), sx.sinc(p["q"], w, p["bins"])
            out = {"intensity": np.array([rs.em.profile(c, f, s) for c in counts])}
            if p["counts"]:
                out["counts"] = counts
            return out
        if entry in ("density_fit", "simulate_density"):
            rho, origin, step, threshold = self.maps[p["map"]]
            E = er.quantise(rho, threshold)[0]
            fits = [rs.em.fit(row, E, origin, step, p["sigma"]) for row in poses]
            if entry == "simulate_density":
                return {"grid": np.array([g for _, g in fits], dtype=np.uint32)}
            return {k: np.array([w[k] for w, _ in fits], dtype=np.uint32 if k == "outside" else np.uint64) for k in ("s", "ss", "se", "inside_sum", "outside")}
        ar = self.assess_restated(call.handle, p["reference"], p["contact"], p["interface"]) if entry in ("assess", "set_reference") else None
        if entry == "assess":
            measures = [ar.measures(row) for row in poses]
            return {"kept": np.array([m["kept"] for m in measures], dtype=np.uint32), "irmsd2": np.array([m["irmsd2"] for m in measures]),
                    "lrmsd2": np.array([m["lrmsd2"] for m in measures]), "_measures": measures, "_rs": ar}
        if entry == "set_reference":
            c = ar.counts()
            return {"counts": np.array([c[k] for k in ("matched_rec", "matched_lig", "native_pairs", "rec_fit", "lig_fit", "interface_fit")], dtype=np.uint32),
                    "native": np.array(ar.native, dtype=np.uint32).reshape(-1, 2)}
        assert entry == "write_pdb"
        text = restated_pdb(rs.em, self.rec_pdb, self.lig_pdb, poses[0])
        return {"text": np.frombuffer(text.encode(), dtype=np.uint8).copy()}

    # -- the library's side -----------------------------------------------------------------------------------------------

    def run(self, pkg, cx, call, scratch):
        """The call on a pkg.Complex of its handle -> {output name: array}; a refusal is the library's LightdockError."""
        p, entry, poses = call.params, call.entry, call.poses
        if entry == "coordinates":
            return {"xyz": cx.coordinates(poses)}
        if entry == "cluster":
            return cx.cluster(poses, call.scores, p["cutoff"])
        if entry == "cluster_ranked":
            return cx.cluster_ranked(poses, call.scores, p["cutoff"], p["atoms"])
        if entry == "contacts":
            return cx.contacts(poses, p["cutoff"])
        if entry == "pair_contacts":
            offsets, keys = cx.pair_contacts(poses, p["cutoff"])
            return {"offsets": offsets, "keys": keys}
        if entry == "cluster_fcc":
            out = cx.cluster_fcc(poses, call.scores, p["cutoff"], p["threshold"], p["min_size"])
            out["n_clusters"] = np.array([out["n_clusters"]], dtype=np.int64)
            return out
        if entry == "sasa":
            return cx.sasa(poses, p["probe"], p["atoms"])
        if entry == "ccs":
            out = cx.ccs(poses, p["what"], p["probe"], p["cell"], p["views"])
            del out["ccs"]                # sums x h^2 / 64e6, made on the host
            return out
        if entry == "crosslinks":
            out = cx.crosslinks(poses, p["links"], p["probe"], p["cell"], p["reach"], p["max_length"], p["paths"])
            del out["straight"]
            return out
        if entry == "distance_histogram":
            return {"counts": cx.distance_histogram(poses, p["width"], p["bins"], p.get("chunk", 0))}
        if entry == "saxs":
            out = cx.saxs(poses, p["q"], p["width"], p["bins"], p["counts"], p.get("chunk", 0))
            return {"intensity": out[0], "counts": out[1]} if p["counts"] else {"intensity": out}
        if entry == "density_fit":
            return cx.density_fit(poses, self.density(pkg, p["map"]), p["sigma"], p.get("chunk", 0))
        if entry == "simulate_density":
            return {"grid": cx.simulate_density(poses, self.density(pkg, p["map"]), p["sigma"], p.get("chunk", 0))}
        if entry in ("assess", "assess_only", "set_reference"):
            if entry != "assess_only":      # assess_only: whatever reference the handle has, or has not
                cx.set_reference(*self.references[p["reference"]], p["contact"], p["interface"])
            if entry != "set_reference":
                out = cx.assess(poses)
                return {"kept": out["kept"], "fnat": out["fnat"], "irmsd": out["irmsd"], "lrmsd": out["lrmsd"]}
            c = cx.reference_counts()
            return {"counts": np.array([c[k] for k in ("matched_rec", "matched_lig", "native_pairs", "rec_fit", "lig_fit", "interface_fit")], dtype=np.uint32),
                    "native": cx.native_pairs()}
        assert entry == "write_pdb"
        path = os.path.join(str(scratch), "history_model.pdb")
        cx.write_pdb(poses[0], path)
        with open(path, "rb") as f:
            return {"text": np.frombuffer(f.read(), dtype=np.uint8).copy()}

    # -- the histories: lists of Step(call, OK or REFUSED) ----------------------------------------------------------------

    def probes(self, handle):
        return [Step(self.call(e, "probe", handle), OK) for e in ENTRIES]

    def soak(self, handle):
        """1. every decoy once: every shared buffer ends larger than any probe needs."""
        return [Step(self.call(e, "decoy", handle), OK) for e in ENTRIES]

    def pair_row(self, handle, x):
        """2. one row: decoy(X), then probe(Y), for every Y."""
        return [step for y in ENTRIES for step in (Step(self.call(x, "decoy", handle), OK), Step(self.call(y, "probe", handle), OK))]

    def pairs(self, handle):
        return [step for x in ENTRIES for step in self.pair_row(handle, x)]

    def refusals(self, handle, how):
        """3. a refused decoy of every entry that has the refusal, every probe after each."""
        out = []
        for e in ENTRIES:
            bad = self.refused(self.call(e, "decoy", handle), how)
            if bad is not None:
                out += [Step(bad, REFUSED)] + self.probes(handle)
        return out

    def refused_reference_history(self, handle):
        """3, the reference: a refused set_reference leaves none, assess is refused, a good one follows."""
        return [Step(self.call("assess", "decoy", handle), OK), Step(self.refused_reference(handle), REFUSED),
                Step(self.call("assess", "probe", handle)._replace(name="%s/assess/without-reference" % handle, entry="assess_only"), REFUSED),
                Step(self.call("set_reference", "probe", handle), OK), Step(self.call("assess", "probe", handle), OK)]

    def flip_history(self, handle):
        """4. inside an entry: options on and off, other sizes, other maps, other references."""
        out = []
        for c in self.flips(handle):
            out.append(Step(c, OK))
            if c.entry == "crosslinks":     # between the flips: the bits out of LDS (the decoy's box), then in it (the probe's)
                out += [Step(self.call("crosslinks", "decoy", handle), OK), Step(self.call("crosslinks", "probe", handle), OK)]
        return out

    def growth(self, handle):
        """5. on a fresh handle (no soak): every probe, every decoy, every probe."""
        return self.probes(handle) + self.soak(handle) + self.probes(handle)

    def two_handles(self):
        """6. both handles, turn by turn, through history 2's first row; the maps are one object for both."""
        rows = [self.pair_row(h, ENTRIES[0]) for h in HANDLES]
        return [step for pair in zip(*rows) for step in pair]


def leading(decoy, probe):
    """The part of a decoy's output that a probe's output of the same name would be, were it read from where the decoy's
    was left: the leading probe.size elements (fewer if the decoy's is smaller), and the probe's cut to as many."""
    d, q = np.asarray(decoy).ravel(), np.asarray(probe).ravel()
    m = min(d.size, q.size)
    return d[:m], q[:m]
