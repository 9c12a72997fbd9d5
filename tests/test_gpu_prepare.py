"""The three kernels of K5 (ld_swarm_diameter2, ld_swarm_shell, ld_swarm_centres; lightdock_hip.h, "Preparing
a run") and prepare.py on the GPU, against tests/setup_reference.py, the rule restated in int64 numpy.  Every decision of
the rule is exact integer arithmetic, so every comparison here is exact equality."""
import ctypes as C
import functools
import glob
import json
import os
import shutil

import numpy as np
import pytest

import setup_reference as sr
from conftest import GOLDEN
from test_analysis_cpu import tool_module

pytestmark = pytest.mark.gpu

LIMIT = 2000000


@pytest.fixture(scope="module")
def gpu(pkg):
    pkg.init(0)
    return pkg


# --- the diameter ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 257, 1000])
def test_diameter(gpu, n):
    rng = np.random.default_rng(n)
    xyz = rng.integers(-60000, 60001, size=(n, 3))
    if n >= 257:   # the extremes twice each, in different workgroups
        xyz[[3, n - 2]] = [-LIMIT, LIMIT, -LIMIT]
        xyz[[130, n - 1]] = [LIMIT, -LIMIT, LIMIT]
    want = sr.diameter2(xyz)
    assert gpu.swarm_diameter2(xyz) == want
    assert want == (0 if n == 1 else 3 * (2 * LIMIT) ** 2 if n >= 257 else int(((xyz[0] - xyz[1]) ** 2).sum()))


def test_diameter_refusals(gpu):
    for bad in (np.zeros((0, 3)), [[0, 0, LIMIT + 1]], [[-LIMIT - 1, 0, 0]]):
        with pytest.raises(gpu.LightdockError) as e:
            gpu.swarm_diameter2(np.array(bad, dtype=np.int64))
        assert e.value.status == -1


# --- the shell ---------------------------------------------------------------------------------------------------------------

def random_atoms(n, seed, box=12000):
    rng = np.random.default_rng(seed)
    radii = rng.choice([1520, 1550, 1700, 1800], size=n)
    return np.concatenate([rng.integers(-box, box + 1, size=(n, 3)), (radii + 3000)[:, None]], axis=1)


SHELL_CASES = {
    "one atom": (np.array([[0, 0, 0, 1700 + 3000]]), None, 2000),
    "two overlapping atoms": (np.array([[0, 0, 0, 4700], [2500, 300, -100, 4550]]), None, 2000),
    "nodes on both spheres": (np.array([[0, 0, 0, 4000]]), None, 2000),
    "all-negative coordinates": (np.array([[-50123, -47001, -39999, 4700], [-52123, -48001, -41999, 4520]]), None, 2000),
    "a lattice of more than 2^16 nodes": (np.array([[100, -200, 300, 40000]]), None, 2000),
    "a bead next to an atom": (np.array([[0, 0, 0, 4700], [5000, 0, 0, 5000]]), np.array([0, 1]), 2000),
    "a corner of the box": (np.array([[LIMIT, -LIMIT, LIMIT, 4700]]), None, 2000),
    "opposite corners": (np.array([[LIMIT, LIMIT, LIMIT, 600000], [-LIMIT, -LIMIT, -LIMIT, 600000]]), None, 500000),
    "an odd spacing": (random_atoms(9, 9), None, 1337),
}
for _n in (1, 63, 64, 65, 257):
    SHELL_CASES["%d atoms" % _n] = (random_atoms(_n, _n), None, 2000)
SHELL_CASES["257 atoms, a third beads"] = (random_atoms(257, 258), np.arange(257) % 3 == 0, 2000)


@functools.lru_cache(maxsize=None)
def shell_reference(name):
    atoms, bead, h = SHELL_CASES[name]
    return sr.shell(atoms, bead, h)


@pytest.mark.parametrize("name", sorted(SHELL_CASES))
def test_shell(gpu, name):
    atoms, bead, h = SHELL_CASES[name]
    want, nodes = shell_reference(name)
    assert gpu.swarm_shell_count(atoms, bead, h) == (len(want), nodes)        # the count-only call
    got = gpu.swarm_shell(atoms, bead, h)                                      # ... and the filling one
    print(name, nodes, "nodes,", len(want), "candidates, %.3f ms" % gpu.setup_last_kernel_ms())
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert len(want) > 0 and [tuple(c) for c in want] == sorted(tuple(c) for c in want)


def test_shell_boundaries_and_beads(gpu):
    atoms, _, h = SHELL_CASES["nodes on both spheres"]
    got = {tuple(c) for c in gpu.swarm_shell(atoms, None, h)}
    assert (4000, 0, 0) in got and (0, -4000, 0) in got       # d^2 = E^2: not inside
    assert (6000, 0, 0) not in got and (0, 0, 6000) not in got and (4000, 4000, 2000) not in got   # d^2 = (E + h)^2: not near
    assert (4000, 4000, 0) in got and (2000, 2000, 2000) not in got
    assert shell_reference("a lattice of more than 2^16 nodes")[1] > 1 << 16
    atoms, bead, h = SHELL_CASES["a bead next to an atom"]
    alone = {tuple(c) for c in gpu.swarm_shell(atoms[:1], None, h)}
    both = {tuple(c) for c in gpu.swarm_shell(atoms, bead, h)}
    assert both < alone and (6000, 0, 0) in alone - both      # the bead removes nodes and adds none
    # beads only: nothing attracts a node; that is no error
    assert gpu.swarm_shell_count(atoms, [1, 1], h)[0] == 0 and gpu.swarm_shell(atoms, [1, 1], h).shape == (0, 3)


# 100 spheres of radius 64 h that do not touch: 2.3e8 nodes, about 5.2e6 shell nodes
CROWD = [[262000 * i - 524000, 262000 * j - 524000, 262000 * k - 393000, 128000] for i in range(5) for j in range(5) for k in range(4)]


def raw_shell(gpu, atoms, spacing, cap, sentinel=-7):
    atoms = np.ascontiguousarray(atoms, dtype=np.int32)
    out = np.full((max(cap, 1), 3), sentinel, dtype=np.int32)
    count, nodes = C.c_size_t(12345), C.c_uint64(777)
    status = gpu.load_library().ld_swarm_shell(atoms.ctypes.data, None, len(atoms), spacing, out.ctypes.data, cap, C.byref(count), C.byref(nodes))
    return status, count.value, nodes.value, out


def test_shell_refusals(gpu):
    atoms = SHELL_CASES["one atom"][0]
    want = len(shell_reference("one atom")[0])
    status, count, nodes, out = raw_shell(gpu, atoms, 2000, want - 1)
    assert status == -1 and count == want and nodes == 777 and np.all(out == -7)       # the count is reported, nothing else
    status, count, nodes, out = raw_shell(gpu, atoms, 2000, want + 3)
    assert status == 0 and count == want and nodes == 729 and np.all(out[want:] == -7) and np.array_equal(out[:want], shell_reference("one atom")[0])
    for bad, spacing, word in (([[0, 0, 0, 4700]], 0, "spacing"), ([[0, 0, 0, 4700]], 1000001, "spacing"), ([[0, 0, 0, 0]], 2000, "extent"),
                               ([[0, 0, 0, 4000001]], 2000, "extent"), ([[LIMIT + 1, 0, 0, 4700]], 2000, "beyond"),
                               ([[0, -LIMIT - 1, 0, 4700]], 2000, "beyond"),
                               ([[LIMIT, LIMIT, LIMIT, 4700], [-LIMIT, -LIMIT, -LIMIT, 4700]], 2000, "spacing"),    # 8e9 nodes
                               (CROWD, 2000, "spacing")):                                                          # more than 2^22 candidates
        status, count, nodes, out = raw_shell(gpu, np.array(bad), spacing, 4)
        assert status == -1 and count == 12345 and nodes == 777 and np.all(out == -7), bad
        assert word in gpu.load_library().ld_last_error().decode(), (bad, gpu.load_library().ld_last_error())
    with pytest.raises(gpu.LightdockError):
        gpu.swarm_shell(np.zeros((0, 4)), None, 2000)


# --- the centres -------------------------------------------------------------------------------------------------------------

def lattice_points(n, seed, box=9, h=2000, offset=(0, 0, 0)):
    rng = np.random.default_rng(seed)
    return rng.integers(-box, box + 1, size=(n, 3)) * h + np.array(offset)


CUBE = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]) * 2000
CENTRE_CASES = {
    "cube, all": (CUBE, 27, 0),
    "cube, more asked than there are": (CUBE, 1000, 0),
    "cube, cover": (CUBE, 27, 2000),
    "one point": (np.array([[5, -7, 9]]), 3, 0),
    "two points": (np.array([[5, -7, 9], [5, -7, 9000]]), 2, 0),
    "two points, covered": (np.array([[5, -7, 9], [5, -7, 9000]]), 2, 9000),
    "1025 points to the last": (lattice_points(1025, 1, box=4), 1025, 0),          # 729 nodes: duplicates, gaps of 0
    "1025 points, fixed count": (lattice_points(1025, 2), 100, 0),
    "1025 points, cover": (lattice_points(1025, 2), 1025, 10000),
    "1025 points, cover beyond the count": (lattice_points(1025, 2), 7, 10000),
    "5000 points, fixed count": (lattice_points(5000, 3, box=30), 300, 0),
    "5000 points, cover": (lattice_points(5000, 3, box=30), 5000, 24000),
    "near the corners": (np.concatenate([lattice_points(300, 4, box=3, offset=(LIMIT - 6000,) * 3),
                                         lattice_points(300, 5, box=3, offset=(-LIMIT + 6000,) * 3),
                                         [[LIMIT, LIMIT, LIMIT], [-LIMIT, -LIMIT, -LIMIT], [LIMIT, LIMIT, LIMIT]]]), 80, 0),
}


@pytest.mark.parametrize("name", sorted(CENTRE_CASES))
def test_centres(gpu, name):
    points, most, cover = CENTRE_CASES[name]
    want_index, want_gap2 = sr.centres(points, most, cover)
    index, gap2 = gpu.swarm_centres(points, most, cover)
    print(name, len(want_index), "centres, %.3f ms" % gpu.setup_last_kernel_ms())
    assert np.array_equal(index, want_index) and np.array_equal(gap2.astype(np.int64), want_gap2)
    assert len(index) == len(set(index.tolist())) >= 1 and np.all(np.diff(want_gap2[1:]) <= 0)
    if cover:
        assert np.all(want_gap2[1:] > cover * cover)
    if name == "cube, all":
        assert index[:4].tolist() == [0, 26, 5, 15]
    if name == "near the corners":
        first, second = np.asarray(points)[index[:2]]
        assert int(want_gap2[1]) == 3 * (2 * LIMIT) ** 2 and np.all(np.abs(first) == LIMIT) and np.array_equal(second, -first)


def test_centres_refusals(gpu):
    lib = gpu.load_library()
    index, gap2, n = np.full(4, 9, dtype=np.uint32), np.full(4, 9, dtype=np.uint64), C.c_size_t(55)
    pts = np.ascontiguousarray(CUBE, dtype=np.int32)
    far = np.array([[0, 0, LIMIT + 1]], dtype=np.int32)
    for p, count, most, cover in ((pts, 27, 0, 0), (pts, 27, 4, -1), (far, 1, 4, 0), (pts, (1 << 22) + 1, 4, 0)):
        assert lib.ld_swarm_centres(p.ctypes.data, count, most, cover, index.ctypes.data, gap2.ctypes.data, C.byref(n)) == -1
        assert n.value == 55 and np.all(index == 9) and np.all(gap2 == 9)
    assert lib.ld_swarm_centres(None, 0, 4, 0, index.ctypes.data, gap2.ctypes.data, C.byref(n)) == 0 and n.value == 0


# --- 1czy, end to end ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def czy_reference():
    g = os.path.join(GOLDEN, "1czy")
    rec, lig = sr.records(os.path.join(g, "lightdock_1czy_protein.pdb")), sr.records(os.path.join(g, "lightdock_1czy_peptide.pdb"))
    t = sr.thousandths_of(lig)[[sr.radius(r) > 0 for r in lig]]
    D = sr.distance(sr.diameter2(t))
    atoms, bead = sr.shell_atoms(rec, D)
    candidates, nodes = sr.shell(atoms, bead, 2000)
    index, gap2 = sr.centres(candidates, 400, 10000)
    ca = [i for i, r in enumerate(rec) if r[12:16].strip() == "CA" and r[21] == "A" and r[17:20] == "SER" and int(r[22:26]) == 467]
    kept = sr.restraint_filter(candidates[index], sr.thousandths_of(rec)[ca[:1]], 20)
    return D, candidates, nodes, index, gap2, kept


def test_1czy_end_to_end(gpu, tmp_path, capsys):
    g = os.path.join(GOLDEN, "1czy")
    shutil.copy(os.path.join(g, "lightdock_1czy_protein.pdb"), tmp_path / "1czy_protein.pdb")
    shutil.copy(os.path.join(g, "lightdock_1czy_peptide.pdb"), tmp_path / "1czy_peptide.pdb")
    tool = tool_module("prepare")
    D, candidates, nodes, index, gap2, kept = czy_reference()
    recs = {s: tool.records(str(tmp_path / f)) for s, f in (("rec", "1czy_protein.pdb"), ("lig", "1czy_peptide.pdb"))}
    found = tool.swarm_centres(gpu, recs["rec"], recs["lig"], 2000, 10000, None, 400)
    print("1czy: D %d, %d nodes, %d candidates, %d centres, %.3f ms" % (found["D"], found["nodes"], len(found["candidates"]), len(found["index"]), found["ms"]))
    assert found["D"] == D == 4697 and found["nodes"] == nodes
    assert np.array_equal(found["candidates"], candidates) and np.array_equal(found["index"], index)
    assert np.array_equal(found["gap2"].astype(np.int64), gap2)
    # LightDock's own ten centres lie near the shell
    worst = 0.0
    for f in sorted(glob.glob(os.path.join(g, "init", "initial_positions_*.dat"))):
        rows = np.array([[float(v) for v in line.split(" ")] for line in open(f).read().splitlines()])
        worst = max(worst, float(np.sqrt(((candidates / 1000.0 - rows[:, :3].mean(axis=0)) ** 2).sum(axis=1)).min()))
    print("1czy: LightDock's centres within %.3f A of a candidate" % worst)
    assert worst <= 6.0

    out = tmp_path / "run"
    argv = [str(tmp_path / "1czy_protein.pdb"), str(tmp_path / "1czy_peptide.pdb"), "-g", "20", "-r", os.path.join(g, "restraints.list"), "--out", str(out)]
    assert tool.main(argv) == 0
    report = capsys.readouterr().out
    print(report)
    assert "D %d, %d nodes, %d candidates, %d centres (%d after the restraint filter)" % (D, nodes, len(candidates), len(index), len(kept)) in report
    setup = json.load(open(out / "setup.json"))
    assert setup["swarms"] == len(kept) and setup["glowworms"] == 20 and setup["receptor_restraints"]["active"] == ["A.SER.467"]
    assert set(json.load(open(os.path.join(g, "setup.json")))) <= set(setup)
    for name in ("1czy_protein.pdb", "1czy_peptide.pdb"):
        assert open(out / ("lightdock_" + name), "rb").read() == open(os.path.join(g, "lightdock_" + name), "rb").read()
    files = sorted(glob.glob(str(out / "init" / "initial_positions_*.dat")))
    assert len(files) == len(kept) and len(open(out / "init" / "swarm_centers.pdb").read().splitlines()) == len(kept)
    centres = candidates[index][kept] / 1000.0
    ser = sr.thousandths_of([r for r in recs["rec"] if r[12:16].strip() == "CA" and r[17:26] == "SER A 467"]) / 1000.0
    for s in (0, len(kept) - 1):
        rows = np.array([[float(v) for v in line.split(" ")] for line in open(out / "init" / ("initial_positions_%d.dat" % s)).read().splitlines()])
        assert rows.shape == (20, 7)
        for k in (0, 19):
            want, _ = sr.pose_row(324324, 20, s, k, list(centres[s]), 10.0, [list(p) for p in ser], [])
            assert np.allclose(rows[k], want, rtol=0, atol=1e-9)
    assert tool.main(argv) == 1                                   # nothing is overwritten
    assert "--force" in capsys.readouterr().err

    # two GSO steps of swarm 0 from the prepared directory
    run_dir = tool_module("run_dir")
    _, setup, sim = run_dir.open_run(str(out / "setup.json"))
    scorer = run_dir.build_scorer(gpu, setup, sim, "dna")
    launch = tool_module("launch")
    pos = launch.read_positions(str(out / "init" / "initial_positions_0.dat"), scorer.pose_len, False)
    gso = gpu.GSO(scorer, pos[None], seeds=[324324])
    gso.run(2)
    assert np.all(np.isfinite(gso.read(0)["scoring"]))
    os.makedirs(out / "swarm_0")
    gso.save(0, 2, str(out / "swarm_0"))
    poses, cols = run_dir.read_gso(str(out / "swarm_0" / "gso_2.out"))
    assert poses.shape[0] == 20 and np.all(np.isfinite(cols["scoring"])) and np.all(np.isfinite(poses))
