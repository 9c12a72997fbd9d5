"""The host half of preparing a run (ld_initial_poses, ld_prepare_pdb, prepare.py's files; lightdock_hip.h, "Preparing a
run") against tests/setup_reference.py, the rule restated in plain Python.  No GPU: the centres these tests
need come from the restatement.

Pose tolerance: 1e-13 max(1, |value|), fewer than 20 roundings of 2^-53 on magnitudes <= 16, plus ln at <= 2 ulp."""
import json
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import setup_reference as sr
from conftest import GOLDEN
from test_analysis_cpu import tool_module

G = 5
REC_POINTS = [[3.25, -1.5, 7.125], [-8.0, 2.75, 0.5], [0.0, 11.0, -4.0]]
LIG_POINTS = [[1.0, 2.0, -0.5], [-3.5, 0.25, 2.0]]


@pytest.fixture(scope="module")
def tool():
    return tool_module("prepare")


def centre_of(s):
    return [12.5 - 3.0 * s, -7.25 + s, 30.0 + 0.125 * s]


def close(got, want):
    return all(abs(a - b) <= 1e-13 * max(1.0, abs(b)) for a, b in zip(got, want))


@pytest.mark.parametrize("anm", [(0, 0), (10, 10), (3, 0)])
@pytest.mark.parametrize("swarm", [0, 7])
@pytest.mark.parametrize("seed", [0, 324324])
def test_pose_rows_match_the_restatement(pkg, seed, swarm, anm):
    assert list(pkg.stdrng_key(seed)) == sr.pcg32_key(seed)
    for rec, lig in (((), ()), (REC_POINTS, LIG_POINTS), (REC_POINTS, ())):
        rows, draws = pkg.initial_poses(seed, G, swarm, centre_of(swarm), rec_points=rec or None, lig_points=lig or None,
                                        anm_rec=anm[0], anm_lig=anm[1])
        assert rows.shape == (G, 7 + sum(anm))
        for g in range(G):
            want, used = sr.pose_row(seed, G, swarm, g, centre_of(swarm), 10.0, rec, lig, anm[0], anm[1])
            assert int(draws[g]) == used, (g, int(draws[g]), used)
            assert close(rows[g], want), (g, rows[g], want)


def test_a_row_is_the_same_bits_alone_or_in_a_batch(pkg):
    batch, draws = pkg.initial_poses(324324, 200, 7, centre_of(7), anm_rec=3, anm_lig=4)
    for g in (0, 1, 63, 199):
        alone, used = pkg.initial_poses(324324, 200, 7, centre_of(7), first=g, n=1, anm_rec=3, anm_lig=4)
        assert alone.tobytes() == batch[g].tobytes() and used[0] == draws[g]
    part, _ = pkg.initial_poses(324324, 200, 7, centre_of(7), first=60, n=10, anm_rec=3, anm_lig=4)
    assert part.tobytes() == batch[60:70].tobytes()
    other, _ = pkg.initial_poses(324324, 200, 8, centre_of(7), anm_rec=3, anm_lig=4)
    assert not np.array_equal(other, batch)


def norm_within(q, eps):
    """| |q| - 1 | <= eps, decided in exact rationals."""
    n2 = sum(Fraction(float(c)) ** 2 for c in q)
    return (1 - Fraction(eps)) ** 2 <= n2 <= (1 + Fraction(eps)) ** 2


@pytest.mark.parametrize("restrained", [False, True])
def test_translations_lie_in_the_swarm_and_rotations_are_unit(pkg, restrained):
    kw = dict(rec_points=REC_POINTS, lig_points=LIG_POINTS) if restrained else {}
    for radius in (10.0, 2.5):
        rows, _ = pkg.initial_poses(11, 200, 3, centre_of(3), radius=radius, **kw)
        d = np.linalg.norm(rows[:, :3] - np.array(centre_of(3)), axis=1)
        assert np.all(d <= radius * (1.0 + 1e-15)) and d.max() > 0.8 * radius
        assert all(norm_within(q, 4.0 * 2.0 ** -53) for q in rows[:, 3:7])


def sine_between(a, b):
    c = np.cross(a, b)
    return np.linalg.norm(c) / (np.linalg.norm(a) * np.linalg.norm(b))


def test_restraint_rotation_turns_the_ligand_residue_to_the_receptor_residue(pkg):
    rows, _ = pkg.initial_poses(5, 64, 2, centre_of(2), rec_points=REC_POINTS, lig_points=LIG_POINTS)
    seen = set()
    for g, row in enumerate(rows):
        want, _ = sr.pose_row(5, 64, 2, g, centre_of(2), 10.0, REC_POINTS, LIG_POINTS)
        t, q = row[:3], row[3:7]
        hits = [(ir, il) for ir, r in enumerate(REC_POINTS) for il, l in enumerate(LIG_POINTS)
                if sine_between(sr.rotate(list(q), l), np.array(r) - t) <= 1e-12 and np.dot(sr.rotate(list(q), l), np.array(r) - t) > 0]
        assert hits, g
        seen.update(hits)
    assert len(seen) == len(REC_POINTS) * len(LIG_POINTS)   # every pair is drawn


@pytest.mark.parametrize("l", [[0.0, 0.0, 2.0], [3.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.5, -2.0, 0.5]])
def test_restraint_rotation_antiparallel_branch(pkg, l):
    """r - t = -k l by construction: radius 0 puts t on the centre, r = centre - 2 l."""
    centre = [4.0, -2.0, 8.0]
    r = [centre[c] - 2.0 * l[c] for c in range(3)]
    rows, _ = pkg.initial_poses(1, 4, 0, centre, radius=0.0, rec_points=[r], lig_points=[l])
    for row in rows:
        q = list(row[3:7])
        assert row[:3].tolist() == centre and q[0] == 0.0 and norm_within(q, 4.0 * 2.0 ** -53)
        turned = sr.rotate(q, l)
        assert sine_between(turned, np.array(r) - row[:3]) <= 1e-12 and np.dot(turned, np.array(r) - row[:3]) > 0
        a = np.array(l) / np.linalg.norm(l)
        axis = min(range(3), key=lambda c: (abs(a[c]), c))
        assert abs(np.dot(q[1:], a)) <= 1e-15 and abs(q[1 + axis]) <= 1e-15   # about a x e: normal to both
        assert close(q, sr.arc_rotation(l, [r[c] - centre[c] for c in range(3)]))


def test_pose_refusals_leave_the_outputs(pkg):
    with pytest.raises(pkg.LightdockError):
        pkg.initial_poses(1, 5, 0, centre_of(0), first=3, n=3)
    with pytest.raises(pkg.LightdockError):
        pkg.initial_poses(1, 5, 0, centre_of(0), radius=-1.0)
    with pytest.raises(pkg.LightdockError):
        pkg.initial_poses(1, 5, 0, [0.0, float("nan"), 0.0])
    with pytest.raises(pkg.LightdockError):
        pkg.initial_poses(1, 5, 0, centre_of(0), rec_points=[[0.0, float("inf"), 0.0]], lig_points=LIG_POINTS)


# --- the cleaner -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lightdock_1czy_protein.pdb", "lightdock_1czy_peptide.pdb"])
def test_cleaner_returns_the_golden_files_byte_for_byte(pkg, tmp_path, name):
    src = os.path.join(GOLDEN, "1czy", name)
    t = sr.thousandths_of(sr.records(src))
    assert np.all(np.abs(t.sum(axis=0)) * 2 < len(t))          # the mean is below 0.0005 A: nothing moves
    atoms, centre = pkg.prepare_pdb(src, str(tmp_path / name))
    assert atoms == len(t) and np.all(np.abs(centre) < 0.0005)
    assert open(tmp_path / name, "rb").read() == open(src, "rb").read()


def pdb_line(serial, name, res, chain, seq, x, y, z, element, het=False):
    return "%-6s%5d %-4s %3s %s%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s" % ("HETATM" if het else "ATOM", serial, name, res, chain, seq, x, y, z, element)


HAND_MADE = [
    "REMARK a hand-made file",
    pdb_line(1, " N", "ALA", "A", 1, 10.0, 0.0, 0.001, "N"),
    pdb_line(2, " CA", "ALA", "A", 1, 11.0, 1.0, 0.002, "C"),
    pdb_line(3, " H", "ALA", "A", 1, 12.0, 2.0, 0.0, "H"),
    pdb_line(4, " OXT", "ALA", "A", 1, 13.0, 3.0, 0.0, "O"),
    pdb_line(5, " O", "HOH", "A", 2, 14.0, 4.0, 0.0, "O", het=True),
    pdb_line(6, " BJ", "MMB", "M", 3, -15.0, 5.0, 0.0, "P", het=True),
    "TER",
    pdb_line(7, "1HB", "ALA", "A", 4, 16.0, 6.0, 0.0, " ")[:60],     # no element field: the name's first letter, H
    "END",
]


@pytest.mark.parametrize("keep", [(False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, True)])
def test_cleaner_keeps_and_drops_by_flag(pkg, tmp_path, keep):
    src = tmp_path / "hand.pdb"
    src.write_text("\n".join(HAND_MADE) + "\n")
    out = tmp_path / "lightdock_hand.pdb"
    atoms, centre = pkg.prepare_pdb(str(src), str(out), *keep)
    want = sr.clean_records(str(src), *keep)
    serials = [int(r[6:11]) for r in want]
    assert serials == sorted({1, 2, 6} | ({3, 7} if keep[0] else set()) | ({4} if keep[1] else set()) | ({5} if keep[2] else set()))
    got = sr.records(str(out))
    assert atoms == len(want) == len(got) and open(out).read() == "".join(r + "\n" for r in got)
    t = sr.thousandths_of(want)
    assert np.array_equal(sr.thousandths_of(got), sr.centred(t))
    assert np.allclose(centre, t.mean(axis=0) / 1000.0, rtol=0, atol=1e-12)
    for a, b in zip(got, want):
        assert a[:30] == b[:30] and a[54:] == b[54:]


def test_cleaner_refuses_a_short_record_and_writes_nothing(pkg, tmp_path):
    src = tmp_path / "short.pdb"
    src.write_text(HAND_MADE[1] + "\n" + HAND_MADE[2][:50] + "\n")
    out = tmp_path / "lightdock_short.pdb"
    with pytest.raises(pkg.LightdockError) as e:
        pkg.prepare_pdb(str(src), str(out))
    assert e.value.status == -3 and not out.exists()
    only_h = tmp_path / "h.pdb"
    only_h.write_text(HAND_MADE[3] + "\n")
    with pytest.raises(pkg.LightdockError) as e:
        pkg.prepare_pdb(str(only_h), str(out))
    assert e.value.status == -1 and not out.exists()
    with pytest.raises(pkg.LightdockError) as e:
        pkg.prepare_pdb(str(tmp_path / "none.pdb"), str(out))
    assert e.value.status == -3


# --- the files of a run ------------------------------------------------------------------------------------------------------

def host_prepared(pkg, tool, tmp_path, case, argv, n_swarms, glowworms):
    """A prepared directory by prepare.py's own host pieces, the centres by the restatement on a coarse lattice (no GPU)."""
    src = os.path.join(GOLDEN, case)
    setup0 = json.load(open(os.path.join(src, "setup.json")))
    args = tool.argument_parser().parse_args(argv)
    restraints = {"rec": dict(setup0["receptor_restraints"]), "lig": dict(setup0["ligand_restraints"])}
    recs = {}
    for side, key in (("rec", "receptor_pdb"), ("lig", "ligand_pdb")):
        out = tmp_path / ("lightdock_" + setup0[key])
        pkg.prepare_pdb(os.path.join(src, "lightdock_" + setup0[key]), str(out), True, True, True)
        recs[side] = tool.records(str(out))
    lig = tool.thousandths(recs["lig"])[tool.radii(recs["lig"]) > 0]
    D = sr.distance(sr.diameter2(lig))
    atoms, bead = tool.shell_atoms(recs["rec"], tool.thousandths(recs["rec"]), D)
    assert np.array_equal(atoms, sr.shell_atoms(recs["rec"], D)[0])
    candidates, _ = sr.shell(atoms, bead, 8000)
    index, _ = sr.centres(candidates, n_swarms)
    centres = candidates[index]
    points = {side: tool.thousandths(recs[side])[tool.restraint_atoms(recs[side], restraints[side]["active"] + restraints[side]["passive"], side)].reshape(-1, 3)
              for side in ("rec", "lig")}
    kept = tool.restraint_filter(centres, points["rec"], args.swarms_per_restraint)
    assert kept == sr.restraint_filter(centres, points["rec"], args.swarms_per_restraint)
    centres = centres[kept] / 1000.0
    anm = (args.anm_rec, args.anm_lig) if args.anm else (0, 0)
    rows = [pkg.initial_poses(args.seed, glowworms, s, centres[s], rec_points=points["rec"] / 1000.0, lig_points=points["lig"] / 1000.0,
                              anm_rec=anm[0], anm_lig=anm[1])[0] for s in range(len(centres))]
    setup = tool.setup_dict(args, setup0["receptor_pdb"], setup0["ligand_pdb"], restraints, len(centres))
    tool.write_run(str(tmp_path), setup, centres, rows)
    return setup, centres, rows


def test_setup_json_round_trips_and_the_oracle_cli_starts_a_run(pkg, orc, tool, tmp_path, monkeypatch):
    setup, centres, rows = host_prepared(pkg, tool, tmp_path, "1azp", ["protein.pdb", "dna.pdb", "-g", "8", "--anm", "--keep-h", "--swarms-per-restraint", "2"], 12, 8)
    assert 1 <= len(centres) <= 6 and setup["swarms"] == len(centres)
    golden = json.load(open(os.path.join(GOLDEN, "1czy", "setup.json")))
    assert set(golden) <= set(setup)
    for key in ("anm_seed", "noh", "anm_rec", "anm_lig", "swarms", "starting_points_seed", "verbose_parser", "noxt", "now", "use_anm",
                "glowworms", "membrane", "receptor_pdb", "ligand_pdb"):
        assert type(setup[key]) is type(golden[key]), key
    run_dir = tool_module("run_dir")
    monkeypatch.setattr(pkg, "init", lambda device=-1: None)     # no GPU here: the file is what is read
    _, read, sim = run_dir.open_run(str(tmp_path / "setup.json"))
    assert read == setup and sim == str(tmp_path)
    # the positions as the reference reads them: single spaces, no trailing blank
    text = open(tmp_path / "init" / "initial_positions_0.dat").read()
    lines = text.splitlines()
    assert len(lines) == 8 and all(len(line.split(" ")) == 27 and line == line.strip() for line in lines)
    assert np.allclose(orc.parse_positions(str(tmp_path / "init" / "initial_positions_0.dat")), rows[0], rtol=0, atol=0.5000001e-9)
    assert len(open(tmp_path / "init" / "swarm_centers.pdb").read().splitlines()) == len(centres)
    # one DNA step of the oracle's CLI from the prepared directory
    for f in ("rec_nm.npy", "lig_nm.npy"):
        shutil.copy(os.path.join(GOLDEN, "1azp", f), tmp_path)
    orc.lib()
    r = subprocess.run([orc.CLI_PATH, "setup.json", os.path.join("init", "initial_positions_0.dat"), "1", "dna"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert r.returncode == 0 and "Creating GSO with 8 glowworms" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    poses, cols = run_dir.read_gso(str(tmp_path / "swarm_0" / "gso_1.out"))
    assert poses.shape == (8, 27) and np.all(np.isfinite(cols["scoring"]))


def test_restraint_filter_and_restraint_atoms(tool):
    recs = [pdb_line(1, " N", "ALA", "A", 1, 0, 0, 0, "N"), pdb_line(2, " CA", "ALA", "A", 1, 1, 0, 0, "C"),
            pdb_line(3, " P", " DT", "B", 13, 2, 0, 0, "P"), pdb_line(4, " O1", "LIG", "C", 5, 3, 0, 0, "O")]
    assert tool.restraint_atoms(recs, ["C.LIG.5", "A.ALA.1", "B.DT.13"], "receptor") == [3, 1, 2]
    with pytest.raises(ValueError, match="A.ALA.2"):
        tool.restraint_atoms(recs, ["A.ALA.2"], "receptor")
    centres = np.array([[0, 0, 0], [2000, 0, 0], [-2000, 0, 0], [0, 9000, 0], [9000, 9000, 0]], dtype=np.int64)
    assert tool.restraint_filter(centres, np.array([[0, 0, 0]]), 2) == [0, 1]                 # 1 and 2 tie: the lower index
    assert tool.restraint_filter(centres, np.array([[0, 0, 0], [9000, 9000, 100]]), 2) == [0, 1, 3, 4]
    assert tool.restraint_filter(centres, np.array([[0, 0, 0]]), 20) == [0, 1, 2, 3, 4]
    parsed = tool.parse_restraints("R A.SER.467 A\nL B.DT.13\n\nR A.ALA.1 P\nL B.DA.2 B\n")
    assert parsed == {"rec": {"active": ["A.SER.467"], "passive": ["A.ALA.1"], "blocked": []},
                      "lig": {"active": ["B.DT.13"], "passive": [], "blocked": ["B.DA.2"]}}


def test_tool_refuses_to_overwrite_before_computing(tool, tmp_path, capsys):
    (tmp_path / "setup.json").write_text("{}")
    assert tool.main(["no_such_rec.pdb", "no_such_lig.pdb", "--out", str(tmp_path)]) == 1
    assert "setup.json" in capsys.readouterr().err and (tmp_path / "setup.json").read_text() == "{}"


def test_restatement_on_hand_cases():
    """The restatement against values worked out by hand."""
    assert sr.diameter2([[0, 0, 0]]) == 0 and sr.diameter2([[0, 0, 0], [3, 4, 12]]) == 169
    assert sr.distance(169) == 3 and sr.distance(4697 * 4697 * 16 + 5) == 4697
    # one atom of extent 4700 at the origin, h = 2000: the axis runs from floor(-6700 / 2000) = -4 to 4
    assert sr.lattice([[0, 0, 0, 4700]], 2000) == [(-4, 9)] * 3
    cand, nodes = sr.shell([[0, 0, 0, 4700]], None, 2000)
    assert nodes == 729
    d2 = (cand ** 2).sum(axis=1)
    assert np.all(d2 >= 4700 ** 2) and np.all(d2 < 6700 ** 2) and len(cand) == len({tuple(c) for c in cand})
    assert [tuple(c) for c in cand] == sorted(tuple(c) for c in cand)
    every = np.array([[i, j, k] for i in range(-4, 5) for j in range(-4, 5) for k in range(-4, 5)]) * 2000
    e2 = (every ** 2).sum(axis=1)
    assert len(cand) == int(((e2 >= 4700 ** 2) & (e2 < 6700 ** 2)).sum())
    cube = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]) * 1000
    index, gap2 = sr.centres(cube, 4)
    # a corner, the opposite corner, then the points with -1, 0 and 1 in some order (5 away from both), lowest index first
    assert index.tolist() == [0, 26, 5, 15] and gap2.tolist() == [3000000, 12000000, 5000000, 5000000]
    assert sorted(sr.centres(cube, 99)[0].tolist()) == list(range(27))
    index, gap2 = sr.centres(cube, 27, cover=1000)
    left = np.setdiff1d(np.arange(27), index)
    assert np.all(gap2[1:] > 1000 ** 2) and all(((cube[index] - cube[i]) ** 2).sum(axis=1).min() <= 1000 ** 2 for i in left)
