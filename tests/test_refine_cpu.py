"""Local refinement without a GPU: the rule's restatement (tests/refine_reference.py) driven by the CPU oracle's energies on
the fixtures, ld_refine_plan's arithmetic and refusals, and the pure functions of lightdock-rust_amd/refine.py.

The counts of TABLE were measured once with the restatement and the oracle; they pin how the rule of lightdock_hip.h "Local
refinement" is read (order of the trials, first maximum, strict acceptance, halving, freezing).  The smallest decision gap
of every row stays above 1e-5, five orders of magnitude above the GPU scorer's error against the oracle (REL_TOL = 1e-9 of
tests/test_gpu_parity.py), so the GPU loop can be held to the same history (tests/test_gpu_refine.py).
"""
import numpy as np
import pytest

from refine_cases import MIN_GAP, TABLE, TABLE_IDS, oracle_refinement, tool_module
import refine_reference as rr


@pytest.mark.parametrize("row", TABLE, ids=TABLE_IDS)
def test_restatement_with_the_oracles_energies(orc, table, row):
    poses, r = oracle_refinement(orc, table, row)
    K, accepted, halvings, frozen, evaluations = row[6:]
    st, hist = r["state"], r["history"]
    assert rr.trial_count(poses.shape[1]) == K
    got = (int(st["accepted"].sum()), int(st["halvings"].sum()), int(st["frozen"].sum()), int(st["evaluations"].sum()))
    print("%s: accepted %d halvings %d frozen %d evaluations %d, smallest gap %.3g" % ((row[0],) + got + (r["min_gap"],)))
    assert got == (accepted, halvings, frozen, evaluations)
    assert r["min_gap"] > MIN_GAP
    assert np.all(r["after"] > r["before"])          # every pose improved
    # the history says the same as the counters
    assert np.array_equal((hist >= 0).sum(axis=1), st["accepted"])
    assert np.array_equal((hist == rr.HALVED).sum(axis=1), st["halvings"])
    assert np.array_equal((hist == rr.FROZEN).sum(axis=1), st["frozen"])
    assert np.array_equal(1 + K * (hist != rr.NOT_EVALUATED).sum(axis=1), st["evaluations"])
    assert hist.max() < K
    for p in range(len(poses)):                      # nothing happens to a pose after it froze
        at = np.flatnonzero(hist[p] == rr.FROZEN)
        if at.size:
            assert np.all(hist[p, at[0] + 1:] == rr.NOT_EVALUATED)


def test_the_half_angle_steps_stay_a_rotation(orc):
    """c and s after h halvings are cos and sin of rot_step / 2^(h + 1) to a few ulp: the rule's formulas, not libm, define them."""
    st = rr.start_state(np.zeros(1), 1.0, 1.0, 0.5)
    for h in range(1, 8):
        rr.halve(st, 0)
        assert abs(st["rot_cos"][0] - np.cos(0.5 / 2 ** h)) < 1e-15 and abs(st["rot_sin"][0] - np.sin(0.5 / 2 ** h)) < 1e-15
        assert st["trans_step"][0] == 2.0 ** -h and st["nm_step"][0] == 0.5 * 2.0 ** -h and st["halvings"][0] == h


# ---------------------------------------------------------------------------------------------------------------------
# ld_refine_plan
# ---------------------------------------------------------------------------------------------------------------------
def workspace_bytes(pose_len, cap, iterations):
    K = 12 + 2 * (pose_len - 7)
    rows = cap * K
    return 8 * (cap * pose_len + rows * pose_len + rows + 6 * cap) + 4 * 3 * cap + 2 * cap * iterations + rows + cap


def test_refine_plan(pkg):
    for pose_len in (7, 8, 27, 73, 135):
        K = 12 + 2 * (pose_len - 7)
        for n in (0, 1, 100, 10 ** 6):
            p = pkg.refine_plan(pose_len, n, pose_len + 3, iterations=20)
            assert p["trials"] == K and p["slice"] == 65536 // K and p["slice"] * K <= 65536
            assert p["workspace_bytes"] == workspace_bytes(pose_len, min(n, p["slice"]), 20)
        p = pkg.refine_plan(pose_len, 100, iterations=3, slice_poses=5)
        assert p["slice"] == 5 and p["workspace_bytes"] == workspace_bytes(pose_len, 5, 3)
    big = pkg.refine_plan(135, 10 ** 6, iterations=20)
    assert big["trials"] == 268 and big["slice"] == 244       # the largest pose a scorer takes
    assert pkg.refine_plan(7, 10, slice_poses=(1 << 22) // 12)["slice"] == (1 << 22) // 12


def test_refine_plan_refusals(pkg):
    import ctypes as C
    lib = pkg.load_library()
    outs = [C.c_size_t(77), C.c_size_t(78), C.c_size_t(79)]

    def call(pose_len, n, stride, iterations, slice_poses):
        return lib.ld_refine_plan(pose_len, n, stride, iterations, slice_poses, *[C.byref(o) for o in outs])

    top = 2 ** 64
    for args in ((6, 1, 7, 1, 0), (136, 1, 136, 1, 0),            # pose_len outside 7 .. 135
                 (27, 1, 26, 1, 0),                               # stride < pose_len
                 (7, 1, 7, 0, 0),                                 # iterations == 0
                 (7, 1, 7, 1, (1 << 22) // 12 + 1),               # slice x K beyond 2^22 rows
                 (135, 1, 135, 1, (1 << 22) // 268 + 1),
                 (7, top // 56 + 1, 7, 1, 0),                     # n x pose_len x 8 (and n x stride x 8)
                 (7, top // 8 // 2 ** 40 + 1, 2 ** 40, 1, 0),     # n x stride x 8 alone
                 (7, top // 2 // 4000000000 + 1, 7, 4000000000, 0),   # n x iterations x 2
                 (7, top - 1, top - 1, 1, 0)):                    # n x stride
        assert call(*args) == -1, args
        assert lib.ld_last_error()
        assert [o.value for o in outs] == [77, 78, 79], args
    assert call(7, top // 56, 7, 1, 0) == 0 and outs[0].value == 12       # the largest n whose arrays a size_t holds
    assert call(7, 0, 7, 1, 0) == 0 and outs[2].value == 0
    assert lib.ld_refine_plan(27, 5, 27, 1, 0, None, None, None) == 0     # any output may be NULL


# ---------------------------------------------------------------------------------------------------------------------
# the tool's pure functions
# ---------------------------------------------------------------------------------------------------------------------
GSO_TEXT = ("#Coordinates  RecID  LigID  Luciferin  Neighbor's number  Vision Range  Scoring\n"
            "(16.3230005, 15.2326313, -1.2815402, -0.1058407, -0.4849369, 0.5997430, -0.6276482, 6.5540618, 6.4979717)"
            "    0    0   -119.26062540  0 0.600 -304.40156350\n"
            "(21.7381997, 13.2379956, 6.2154227, -0.3588059, -0.4977777, -0.7363521, 0.2850636, 5.4210282, 6.3518031)"
            "    0    0   8.96966174  0 0.600 16.17415435\n"
            "(1.5, 2.5, 3.5, 1.0, 0.0, 0.0, 0.0, 0.25, 0.75)    0    0   1.00000000  3 0.200 2.50000000\n")


def test_rewritten_gso_file_returns_the_refined_doubles(tmp_path):
    tool, run_dir = tool_module("refine"), tool_module("run_dir")
    rng = np.random.default_rng(5)
    pose7 = rng.standard_normal(7) * np.pi            # 7 of the 9 coordinates: the other two keep their text
    pose9 = rng.standard_normal(9) / 3.0
    refined = {0: (pose7, -1.0 / 3.0), 2: (pose9, 1e-300 * np.pi)}
    text = tool.rewrite_gso(GSO_TEXT, refined)
    path = tmp_path / "gso_1.out"
    path.write_text(text)
    poses, cols = run_dir.read_gso(str(path))
    (tmp_path / "orig.out").write_text(GSO_TEXT)
    before, cols0 = run_dir.read_gso(str(tmp_path / "orig.out"))
    assert np.array_equal(poses[0, :7], pose7) and np.array_equal(poses[0, 7:], before[0, 7:])
    assert np.array_equal(poses[2], pose9)
    assert cols["scoring"][0] == -1.0 / 3.0 and cols["scoring"][2] == 1e-300 * np.pi
    for k in ("rec_id", "lig_id", "luciferin", "neighbors", "vision_range"):
        assert np.array_equal(cols[k], cols0[k])
    # untouched rows and columns are the same bytes
    old, new = GSO_TEXT.splitlines(keepends=True), text.splitlines(keepends=True)
    assert len(old) == len(new) and new[0] == old[0] and new[2] == old[2]
    for k in (1, 3):
        o_inner, o_rest = old[k][1:].split(")", 1)
        n_inner, n_rest = new[k][1:].split(")", 1)
        assert n_rest[:n_rest.rstrip().rfind(" ") + 1] == o_rest[:o_rest.rstrip().rfind(" ") + 1] and n_rest.endswith("\n")
    assert new[1][1:].split(")")[0].split(",")[7:] == old[1][1:].split(")")[0].split(",")[7:]
    assert tool.rewrite_gso(GSO_TEXT, {}) == GSO_TEXT
    with pytest.raises(ValueError):
        tool.rewrite_gso(GSO_TEXT, {3: (pose7, 0.0)})
    with pytest.raises(ValueError):
        tool.rewrite_gso(GSO_TEXT, {0: (np.zeros(10), 0.0)})


def test_refined_list_parses_and_is_sorted():
    tool, decompose = tool_module("refine"), tool_module("decompose")
    rng = np.random.default_rng(6)
    n = 5
    poses = rng.standard_normal((n, 9))
    poses[:, 3:7] /= np.linalg.norm(poses[:, 3:7], axis=1)[:, None]
    refined = poses.copy()
    refined[1, :3] += (3.0, 4.0, 12.0)                                              # moved 13 A
    refined[2, 3:7] = [np.cos(0.25), np.sin(0.25), 0.0, 0.0]                         # turned 0.5 rad from the identity
    poses[2, 3:7] = [1.0, 0.0, 0.0, 0.0]
    refined[3, 3:7] = -2.5 * poses[3, 3:7]                                           # the same rotation
    stats = np.zeros(n, dtype=[("energy_before", "f8"), ("energy_after", "f8"), ("accepted", "u4"), ("halvings", "u4"),
                               ("evaluations", "u4"), ("frozen", "u4")])
    stats["energy_before"] = [1.0, -2.0, 3.0, 0.5, np.pi]
    stats["energy_after"] = [1.5, 7.25, 3.0, 0.5 + 1e-9, np.pi]
    stats["accepted"], stats["halvings"], stats["evaluations"] = [1, 9, 0, 2, 0], [0, 1, 4, 4, 4], [241, 241, 61, 241, 61]
    entries = [(k % 2, 10 + k, poses[k], {"scoring": 0.1 * k}) for k in range(n)]
    rows = tool.refined_rows(entries, poses, refined, stats)
    assert [r[10] for r in rows] == [1, 4, 2, 0, 3]
    text = tool.refined_text(rows)
    for parse in (tool.parse_list, decompose.parse_list):                           # both lists' parsers read it
        head, body = parse(text)
        assert head == tool.REFINED_HEADER.split() and len(body) == n and all(len(x) == len(head) for x in body)
    col = {h: k for k, h in enumerate(head)}
    after = [float(x[col["After"]]) for x in body]
    assert after == sorted(after, reverse=True) and after == [7.25, np.pi, 3.0, 1.5, 0.5 + 1e-9]     # 17 digits: the doubles
    assert [int(x[col["Glowworm"]]) for x in body] == [11, 14, 12, 10, 13]
    assert abs(float(body[0][col["Moved"]]) - 13.0) < 1e-5 and abs(float(body[2][col["Turned"]]) - 0.5) < 1e-6
    assert float(body[4][col["Turned"]]) < 1e-6 and float(body[3][col["Moved"]]) == 0.0
    assert np.isnan(tool.turned(np.zeros(7), poses[0]))
