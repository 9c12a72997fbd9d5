"""Clustering of one ranked list across swarms (ld_complex_cluster_ranked, lightdock-rust_amd/cluster_run.py, DESIGN §5
K3e) on the CPU: the script's candidate gathering and its two text formats on the committed 1czy run, and an int64 numpy
restatement of the rule (the checker the GPU tests use), held against Restated.bsas of tests/test_analysis_cpu.py."""
import os

import numpy as np

from test_analysis_cpu import CZY, ROOT, Restated, analyse_module, czy_restated, tool_module


def cluster_run_module():
    return tool_module("cluster_run")


# ---- int64 numpy restatement of the rule ------------------------------------------------------------------------------

def printed_thousandths(x):
    """The integer c with "%.3f" % x == c / 1000, elementwise, as int64.  rint(x * 1000) unless the product is within 1e-6
    of a half, where the decimal string itself decides."""
    x = np.asarray(x, dtype=np.float64)
    p = x * 1000.0
    out = np.rint(p)
    frac = p - np.floor(p)
    for idx in zip(*np.nonzero(np.abs(frac - 0.5) < 1e-6)):
        out[idx] = round(float("%.3f" % x[idx]) * 1000.0)
    assert np.all(np.abs(out) < 2.0 ** 31)
    return out.astype(np.int64)


class RankedRestated:
    """The rule of lightdock_hip.h, "Clustering a ranked list", over a tests/test_analysis_cpu.py Restated complex."""

    def __init__(self, restated):
        self.rs = restated
        self.n_rec = len(restated.rec)
        bb = np.asarray(restated.backbone, dtype=np.int64)
        self.atoms = {"complex": bb, "ligand": bb[bb >= self.n_rec]}

    def posed(self, poses, atoms):
        """Restated.pose for all poses at once, the chosen atoms only: (n, len(atoms), 3) f64, the same operations in
        the same order per element."""
        rs, poses = self.rs, np.asarray(poses, dtype=np.float64)
        na, nl = len(rs.rec_modes), len(rs.lig_modes)
        rec_atoms, lig_atoms = atoms[atoms < self.n_rec], atoms[atoms >= self.n_rec] - self.n_rec
        r = np.broadcast_to(rs.rec[rec_atoms], (len(poses), len(rec_atoms), 3)).copy()
        for m in range(na):
            r = r + rs.rec_modes[m][rec_atoms][None] * poses[:, 7 + m, None, None]
        v = np.broadcast_to(rs.lig[lig_atoms], (len(poses), len(lig_atoms), 3)).copy()
        for m in range(nl):
            v = v + rs.lig_modes[m][lig_atoms][None] * poses[:, 7 + na + m, None, None]
        qw, qx, qy, qz = (poses[:, k, None] for k in (3, 4, 5, 6))
        vx, vy, vz = v[:, :, 0], v[:, :, 1], v[:, :, 2]
        aw = qw * 0.0 - qx * vx - qy * vy - qz * vz
        ax = qw * vx + qx * 0.0 + qy * vz - qz * vy
        ay = qw * vy - qx * vz + qy * 0.0 + qz * vx
        az = qw * vz + qx * vy - qy * vx + qz * 0.0
        n2 = qw * qw + qx * qx + qy * qy + qz * qz
        bw, bx, by, bz = qw / n2, -qx / n2, -qy / n2, -qz / n2
        lig = np.stack([aw * bx + ax * bw + ay * bz - az * by + poses[:, 0, None],
                        aw * by - ax * bz + ay * bw + az * bx + poses[:, 1, None],
                        aw * bz + ax * by - ay * bx + az * bw + poses[:, 2, None]], axis=2)
        return np.concatenate([r, lig], axis=1)

    def thousandths(self, poses, atoms="complex"):
        """(n, 3 x atoms) int64: what "%.3f" prints of the posed atoms, times 1000."""
        return printed_thousandths(self.posed(poses, self.atoms[atoms])).reshape(len(poses), 3 * len(self.atoms[atoms]))

    def cluster(self, poses, scoring, cutoff=4.0, atoms="complex"):
        """(cluster_of, representatives, knife): poses by (scoring descending, index ascending); each joins the first
        representative in creation order with rint(sqrt(S * 1e-6 / n_atoms) * 1e4) / 1e4 <= cutoff, else founds a cluster.
        S: the int64 sum of squared differences of the thousandths (|a|^2 + |b|^2 - 2 a.b in int64, exact).  knife: the
        comparisons, against EVERY representative, whose rmsd * 1e4 is within 1e-9 of a .5."""
        T = self.thousandths(poses, atoms)
        n, n_atoms = len(T), T.shape[1] // 3
        scoring = np.asarray(scoring, dtype=np.float64)
        sq = (T * T).sum(axis=1)
        assert n == 0 or 4 * int(sq.max()) < 2 ** 62   # no int64 sum below can wrap
        order = sorted(range(n), key=lambda i: -scoring[i])   # stable: ties in index order
        R = np.empty_like(T)
        Rsq = np.empty(n, dtype=np.int64)
        reps, cluster_of, knife = [], np.full(n, -1, dtype=np.int64), 0
        for i in order:
            k = len(reps)
            S = Rsq[:k] + sq[i] - 2 * (R[:k] @ T[i])
            x = np.sqrt(S * 1e-6 / n_atoms) * 1e4
            knife += int((np.abs(x - np.floor(x) - 0.5) < 1e-9).sum())
            near = np.flatnonzero(np.rint(x) / 1e4 <= cutoff)
            if len(near):
                cluster_of[i] = near[0]
            else:
                cluster_of[i] = k
                R[k], Rsq[k] = T[i], sq[i]
                reps.append(i)
        return cluster_of, reps, knife


def czy_run(swarms=range(10)):
    """The committed 1czy run's gso_100.out of the given swarms as one list: (poses (n, 27), scoring (n,))."""
    an = analyse_module()
    runs = [an.read_gso(os.path.join(CZY, "swarm_%d" % s, "gso_100.out")) for s in swarms]
    return np.concatenate([p for p, _ in runs]), np.concatenate([c["scoring"] for _, c in runs])


# ---- tests ------------------------------------------------------------------------------------------------------------

def test_printed_thousandths_are_the_decimal_string():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-300, 300, 2000), np.arange(-40, 40) / 16.0 + 0.0005, [0.0005, 1.0005, 2.5, -0.0005, 1e-9, -1e-9]])
    want = [round(float("%.3f" % v) * 1000.0) for v in x]
    assert list(printed_thousandths(x)) == want


def test_restatement_agrees_with_restated_bsas_on_the_2000_golden_poses():
    """The ten swarms of the committed 1czy run as one list, under the per-swarm rule's own restatement: 7 clusters, where
    the ten cluster.repr files hold 11 representatives; no knife-edge comparison on either side."""
    rs = czy_restated()
    poses, scoring = czy_run()
    assert poses.shape == (2000, 27)
    want_of, want_reps, want_knife = rs.bsas(poses, scoring, 4.0)
    got_of, got_reps, knife = RankedRestated(rs).cluster(poses, scoring, 4.0, "complex")
    assert want_knife == 0 and knife == 0
    assert len(want_reps) == 7 and got_reps == want_reps and np.array_equal(got_of, want_of)
    n_repr = sum(len(list(filter(str.strip, open(os.path.join(CZY, "swarm_%d" % s, "cluster.repr"))))) for s in range(10))
    assert n_repr == 11
    # the posing itself, all poses at once, against the one-pose restatement
    rr = RankedRestated(rs)
    for k in (0, 777, 1999):
        assert np.array_equal(rr.posed(poses[k:k + 1], rr.atoms["complex"])[0], rs.pose(poses[k])[rs.backbone])


def test_restatement_on_one_swarm_and_under_the_ligand_measure():
    rs = czy_restated()
    rr = RankedRestated(rs)
    poses, scoring = czy_run([9])
    want_of, want_reps, _ = rs.bsas(poses, scoring, 4.0)
    got_of, got_reps, knife = rr.cluster(poses, scoring, 4.0)
    assert knife == 0 and got_reps == want_reps and np.array_equal(got_of, want_of) and len(got_reps) == 2
    assert len(rr.atoms["complex"]) == 175 and len(rr.atoms["ligand"]) == 7
    # the receptor dilutes BSAS's measure: the same poses fall apart under the ligand's own atoms
    lig_of, lig_reps, _ = rr.cluster(poses, scoring, 4.0, "ligand")
    assert len(lig_reps) > len(got_reps)
    # rigid, identity rotations: the ligand's RMSD is the distance of the translations
    rigid = RankedRestated(Restated(os.path.join(CZY, "lightdock_1czy_protein.pdb"), os.path.join(CZY, "lightdock_1czy_peptide.pdb")))
    chain = np.zeros((6, 7))
    chain[:, 3] = 1.0
    chain[:, 0] = 3.0 * np.arange(6)
    of, reps, _ = rigid.cluster(chain, -np.arange(6.0), 4.0, "ligand")
    assert reps == [0, 2, 4] and list(of) == [0, 0, 1, 1, 2, 2]   # an absorbed pose leads nobody
    assert rigid.cluster(chain[:0], np.zeros(0), 4.0)[1] == []


def test_script_gathers_the_candidates_of_filter_py_and_formats_both_lists():
    cr, an = cluster_run_module(), analyse_module()
    ranked = cr.candidates(range(10), 100, base=CZY)
    assert [(e[0], e[1]) for e in ranked] == [(e[0], e[1]) for e in an.ranking(range(10), 100, base=CZY)] and len(ranked) == 11
    every = cr.candidates(range(10), 100, every=True, base=CZY)
    assert len(every) == 2000
    keys = [(-e[3]["scoring"], e[0], e[1]) for e in every]
    assert keys == sorted(keys)
    poses, scoring = czy_run()
    by_pose = {(s, g): poses[200 * s + g] for s in range(10) for g in range(200)}
    assert all(np.array_equal(e[2], by_pose[e[0], e[1]]) for e in every[:50] + ranked)

    rr = RankedRestated(czy_restated())
    for entries in (ranked, every):
        p = np.array([e[2] for e in entries])
        s = np.array([e[3]["scoring"] for e in entries])
        of, reps, knife = rr.cluster(p, s, 4.0)
        assert knife == 0
        text = cr.rank_clustered_text(entries, of, reps + [-1] * (len(entries) - len(reps)), len(reps))
        lines = text.splitlines()
        assert lines[0] + "\n" == cr.CLUSTERED_HEADER and len(lines) == 1 + len(reps)
        rows = [l.split() for l in lines[1:]]
        assert [int(r[0]) for r in rows] == list(range(len(reps)))
        assert sum(int(r[1]) for r in rows) == len(entries)
        assert [float(r[4]) for r in rows] == sorted((float(r[4]) for r in rows), reverse=True)   # best scoring first
        assert rows[0][2:] == [str(entries[0][0]), str(entries[0][1]), "%.5f" % entries[0][3]["scoring"]]
        members = cr.members_text(entries, of).splitlines()
        assert members[0] + "\n" == cr.MEMBERS_HEADER and len(members) == 1 + len(entries)
        assert members[1].split() == ["0", str(entries[0][0]), str(entries[0][1]), "%.5f" % entries[0][3]["scoring"]]
        assert [int(m.split()[0]) for m in members[1:]] == list(of)
    assert len(reps) == 7   # every glowworm of the ten swarms: 7 clusters
    # fixed-width columns
    one = cr.rank_clustered_text([(3, 17, None, {"scoring": 12.3456789})], [0], [0], 1)
    assert one == cr.CLUSTERED_HEADER + "      0       1      3        17    12.34568\n"
    assert cr.members_text([(3, 17, None, {"scoring": -1.5})], [0]) == cr.MEMBERS_HEADER + "      0      3        17    -1.50000\n"
