"""lightdock-rust_amd/run_dir.py, what the post-run tools share, on the CPU: the pose matrix, the Complex of a run against
a stand-in package, the swarm list, the candidate lists on the committed 1czy run and on a small made-up one, and which
tool imports what."""
import ast
import json
import os

import numpy as np
import pytest

from test_analysis_cpu import CZY, ROOT, tool_module
from test_contacts_cpu import two_swarm_run

TOOLS = ("analyse", "filter", "assess", "cluster_run", "decompose")


def same_entries(a, b):
    return len(a) == len(b) and all(x[:2] == y[:2] and np.array_equal(x[2], y[2]) and x[3] == y[3] for x, y in zip(a, b))


def test_pose_matrix_is_the_expression_it_replaces():
    rd = tool_module("run_dir")
    entries = rd.ranking(range(10), 100, base=CZY)
    assert len(entries) == 11 and len(entries[0][2]) == 27
    for pose_len in (27, 7):
        want = np.array([e[2][:pose_len] for e in entries]).reshape(len(entries), pose_len)
        got = rd.pose_matrix(entries, 100, pose_len)
        assert got.shape == (11, pose_len) and got.dtype == want.dtype and np.array_equal(got, want)
    short = list(entries)
    short[4] = (short[4][0], short[4][1], short[4][2][:26], short[4][3])
    with pytest.raises(ValueError) as err:
        rd.pose_matrix(short, 100, 27)
    assert str(err.value) == "gso_100.out must hold poses of at least 27 columns"
    assert rd.pose_matrix(short, 100, 26).shape == (11, 26)
    none = rd.pose_matrix([], 100, 27)
    assert none.shape == (0, 27) and none.dtype == np.float64


class RecordingPackage:
    """A stand-in for the package: its Complex keeps what it was built with."""

    class Complex:
        def __init__(self, rec, lig, **kw):
            self.rec, self.lig, self.kw = rec, lig, kw


@pytest.mark.parametrize("use_anm,anm_rec,anm_lig,sides", [(False, 10, 10, ()), (True, 10, 0, ("rec",)), (True, 10, 4, ("rec", "lig"))])
def test_complex_of_a_run(tmp_path, monkeypatch, use_anm, anm_rec, anm_lig, sides):
    rd = tool_module("run_dir")
    sim, cwd = tmp_path / "sim", tmp_path / "cwd"
    os.makedirs(sim)
    os.makedirs(cwd)
    setup = {"use_anm": use_anm, "anm_rec": anm_rec, "anm_lig": anm_lig, "receptor_pdb": "r.pdb", "ligand_pdb": "l.pdb", "swarms": 3}
    with open(sim / "setup.json", "w") as f:
        json.dump(setup, f)
    modes = {"rec": np.arange(10 * 5 * 3, dtype=np.float64).reshape(10, 5, 3), "lig": -np.arange(4 * 2 * 3, dtype=np.float64)}
    for side in sides:      # only the files a side with modes reads: another side's would be a FileNotFoundError
        np.save(cwd / ("%s_nm.npy" % side), modes[side])
    monkeypatch.chdir(cwd)
    cx = rd.build_complex(RecordingPackage, json.load(open(sim / "setup.json")), str(sim))
    assert (cx.rec, cx.lig) == (os.path.join(str(sim), "lightdock_r.pdb"), os.path.join(str(sim), "lightdock_l.pdb"))
    assert sorted(cx.kw) == sorted(["rec_num_anm", "lig_num_anm"] + [s + "_nmodes" for s in sides])
    assert (cx.kw["rec_num_anm"], cx.kw["lig_num_anm"]) == ((anm_rec, anm_lig) if use_anm else (0, 0))
    for side in sides:
        got = cx.kw[side + "_nmodes"]
        assert got.ndim == 1 and got.dtype == np.float64 and np.array_equal(got, modes[side].reshape(-1))


def test_swarm_list():
    rd = tool_module("run_dir")
    assert rd.swarm_list(None, {"swarms": 4}) == [0, 1, 2, 3] == list(range(4))
    assert rd.swarm_list("0-2,7", {"swarms": 4}) == [0, 1, 2, 7]


def test_candidates_are_the_ranking_or_every_glowworm(tmp_path):
    rd = tool_module("run_dir")
    two_swarm_run(tmp_path)
    for s, reps in ((0, (1, 0)), (3, (2,))):
        with open(tmp_path / ("swarm_%d" % s) / "cluster.repr", "w") as f:
            f.writelines("%d:1: 0.00000:%d:lightdock_%d.pdb\n" % (c, g, g) for c, g in enumerate(reps))
    for swarms, step, base, n_ranked, n_all in ((range(10), 100, CZY, 11, 2000), ([3, 0], 5, str(tmp_path), 3, 6)):
        ranked, every = rd.candidates(swarms, step, every=False, base=base), rd.candidates(swarms, step, every=True, base=base)
        assert same_entries(ranked, rd.ranking(swarms, step, base=base)) and len(ranked) == n_ranked
        assert same_entries(every, rd.all_glowworms(swarms, step, base=base)) and len(every) == n_all
        assert same_entries(rd.candidates(swarms, step, base=base), ranked)      # the ranking is the default
    assert [e[:2] for e in rd.candidates([3, 0], 5, base=str(tmp_path))] == [(0, 1), (3, 2), (0, 0)]


def test_every_name_is_where_tools_and_tests_look_for_it():
    rd = tool_module("run_dir")
    an, fl, cr = tool_module("analyse"), tool_module("filter"), tool_module("cluster_run")
    for mod, names in ((an, ("read_gso", "ranking")), (fl, ("all_glowworms",)), (cr, ("candidates",))):
        for name in names:
            assert getattr(mod, name).__module__.endswith("run_dir") and hasattr(rd, name)


def imported_modules(path):
    """The last component of every module an import statement of the file names."""
    found = set()
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Import):
            found.update(a.name.split(".")[-1] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            found.update([node.module.split(".")[-1]] if node.module else [a.name for a in node.names])
    return found


def test_tools_import_run_dir_and_only_the_filter_imports_filter():
    tools = os.path.join(ROOT, "lightdock-rust_amd")
    for name in TOOLS:
        assert "run_dir" in imported_modules(os.path.join(tools, name + ".py")), name
    for f in sorted(os.listdir(tools)):
        if f.endswith(".py") and f != "filter.py":
            assert "filter" not in imported_modules(os.path.join(tools, f)), f
