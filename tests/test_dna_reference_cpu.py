"""tests/dna_reference.py held to the oracle, and the conditions on the inputs of tests/test_gpu_dna_pairs.py, on the CPU.

The restatement and the oracle are two readings of src/dna.rs:471-512 and src/scoring.rs:21-47; the 1azp fixture with its
restraints and normal modes holds one to the other, so that the GPU suite's reference does not share a misreading with
the kernel.  The conditions (a)-(d) are what makes the derived bound a check: finite, NaN only where the reference has
one, every clamp and cutoff reached, and far below the size of one pair at the cutoff."""
import numpy as np

import dna_reference as dr
from conftest import case_kwargs, case_positions

U = dr.U


def test_restatement_against_the_oracle_on_1azp(orc):
    """energy, elec, vdw within 2 P u sum|t| of the oracle's sequential sums (two f64 sums of the same P terms in different
    association; the exact sum errs by nothing, the sequential one by at most (P - 1) u sum|t| to first order), the tail
    carried along as (1 + fr + fl) and 8 u |E| for its roundings; counts and fractions exactly."""
    method, rec_pdb, lig_pdb, kw = case_kwargs("1azp", orc, None)
    assert method == "dna" and kw["use_anm"]
    cpu = orc.Scorer(method, rec_pdb, lig_pdb, **kw)
    rec, lig = cpu.model(0), cpu.model(1)
    for mol, tag in ((rec, "rec"), (lig, "lig")):
        mol["modes"] = np.asarray(kw[tag + "_nmodes"], dtype=np.float64).reshape(kw[tag + "_num_anm"], -1, 3)
    assert rec["restraint_offsets"].size == 4 and lig["restraint_offsets"].size == 2
    poses = case_positions("1azp", orc)[:12]
    assert len(poses) == 12
    fractions = set()
    for p, row in enumerate(poses):
        want = dr.dna_reference(orc, rec, lig, row, kw["rec_num_anm"], kw["lig_num_anm"])
        energy, stats = cpu.energy_ex_row(row)
        assert energy == cpu.energy_row(row) and not want["nan"]
        tail = 1.0 + want["rec_restraints"] + want["lig_restraints"]
        b_elec = 2.0 * want["P"][0] * U * want["abs_terms"][0] / (332.0 / 4.0)
        b_vdw = 2.0 * want["P"][1] * U * want["abs_terms"][1]
        bound = 2.0 * want["P"][0] * U * sum(want["abs_terms"]) * tail + 8.0 * U * abs(want["energy"])
        print("1azp pose %d: energy %.17g oracle %.17g |diff| %.3g bound %.3g" % (p, want["energy"], energy, abs(want["energy"] - energy), bound))
        assert abs(want["energy"] - energy) <= bound
        assert abs(want["elec"] - stats[0]) <= b_elec and abs(want["vdw"] - stats[1]) <= b_vdw
        assert want["rec_restraints"] == stats[2] and want["lig_restraints"] == stats[3] and want["membrane"] == stats[4]
        assert want["pairs"] == int(stats[5])
        assert int(want["rec_interface"].sum()) == int(stats[6]) and int(want["lig_interface"].sum()) == int(stats[7])
        assert 0.0 < want["bound"] < np.inf
        fractions.add((want["rec_restraints"], want["lig_restraints"]))
    assert len(fractions) > 1          # the tail is not the same for all twelve


def all_cases(orc):
    """(name, n_rec, n_lig, poses, references) of everything tests/test_gpu_dna_pairs.py compares with the restatement."""
    for shape in dr.SHAPES:
        _, _, poses, want = dr.shape_reference(orc, shape)
        yield dr.shape_id(shape), shape[0], shape[1], poses, want
    _, _, poses, want = dr.tail_case(orc)
    yield "tail", dr.TAIL_SHAPE[0], dr.TAIL_SHAPE[1], poses, want
    for shape in dr.ANM_SHAPES:
        for k_rec, k_lig in dr.ANM_MODES:
            _, _, poses, want = dr.anm_case(orc, shape, k_rec, k_lig)
            yield "anm %s (%d, %d)" % (dr.shape_id(shape), k_rec, k_lig), shape[0], shape[1], poses, want


def test_conditions_on_the_inputs_of_the_gpu_tests(orc):
    for name, n_rec, n_lig, poses, want in all_cases(orc):
        assert len(want) == len(poses) and dr.N_SPECIAL < len(poses) <= 39
        # (a) the bound is finite wherever the reference is, and positive wherever a pair is inside the cutoff (with no pair
        #     inside it the bound is 0.0: the kernel has to return the reference's zero exactly)
        for p, w in enumerate(want):
            if not w["nan"]:
                assert np.isfinite(w["bound"]) and np.isfinite(w["energy"]), (name, p)
                assert w["bound"] > 0.0 if w["pairs"] else w["bound"] == 0.0, (name, p)
        # (b) NaN for the coincident atoms only (normal modes move them apart)
        nans = [p for p, w in enumerate(want) if w["nan"]]
        assert nans == ([] if name.startswith("anm") else [dr.ROW_COINCIDENT]), (name, nans)
        assert all(np.isnan(want[p]["energy"]) and np.isnan(want[p]["bound"]) for p in nans)
        # (c) every clamp, both cutoffs and the interface occur
        if n_rec >= 64 and n_lig >= 64:
            for what in ("e_high", "e_low", "k_clamped", "k_negative", "between", "beyond", "interface"):
                assert sum(w["seen"][what] for w in want) >= 1, (name, what)
        # (d) a pair wrongly dropped at the cutoff stays a thousand bounds away
        if n_rec >= 2 and n_lig >= 2:
            near = np.concatenate([w["near_cutoff"] for w in want])
            assert near.size > 0, name
            worst = max(w["bound"] for w in want if not w["nan"])
            print("%s: largest bound %.3g, median pair at the cutoff %.3g" % (name, worst, np.median(near)))
            assert worst < 1e-3 * np.median(near), name

    assert [len(dr.shape_poses(s)) for s in dr.SHAPES] == [39, 39, 39, 39, 39, 39, 14, 39, 39, 39, 14]

    # the special rows are what they are said to be, on the one pair of 1 x 1
    _, _, _, one = dr.shape_reference(orc, dr.SHAPES[0])
    assert dr.SHAPES[0][:2] == (1, 1)
    pairs = [one[r]["pairs"] for r in (dr.ROW_225, dr.ROW_FAR, dr.ROW_900, dr.ROW_100, dr.ROW_IFACE, dr.ROW_OUTSIDE_900, dr.ROW_OUTSIDE_100)]
    assert pairs == [1, 0, 1, 1, 1, 0, 1]
    assert one[dr.ROW_900]["energy"] != 0.0 and one[dr.ROW_900]["vdw"] == 0.0
    assert one[dr.ROW_100]["vdw"] != 0.0 and one[dr.ROW_OUTSIDE_100]["vdw"] == 0.0 and one[dr.ROW_OUTSIDE_100]["elec"] != 0.0
    assert one[dr.ROW_IFACE]["rec_interface"].all() and not one[dr.ROW_100]["rec_interface"].any()
    assert one[dr.ROW_FAR]["energy"] == 0.0 and one[dr.ROW_OUTSIDE_900]["energy"] == 0.0

    # the tail case reaches every fraction the issue names, on poses that are not NaN
    _, _, _, tail = dr.tail_case(orc)
    live = [w for w in tail if not w["nan"]]
    assert {w["rec_restraints"] for w in live} == {0.0, 0.5, 1.0} and {w["lig_restraints"] for w in live} == {0.0, 1.0}
    assert any(w["membrane"] > 0.0 for w in live) and any(w["membrane"] == 0.0 for w in live)


def test_the_bound_catches_a_broken_kernel_on_64x64(orc):
    """Three ways to break the kernel, emulated on the reference's own terms of the 64 x 64 shape: no Newton step after the
    reciprocal (1 / d2 only as good as f32), `<` for `<=` at 900, the van der Waals clamp at 2 instead of 1.  Each has to
    move some pose's energy by more than its bound."""
    shape = dr.SHAPES[2]
    assert shape[:2] == (64, 64)
    rec, lig, poses, want = dr.shape_reference(orc, shape)
    caught = {"rcp": 0, "cutoff": 0, "clamp": 0}
    for p, row in enumerate(poses):
        if want[p]["nan"]:
            continue
        t = dr.dna_reference(orc, rec, lig, row, n_chunks=shape[3], keep_terms=True)["terms"]
        d2, cut, cut_vdw = t["d2"], t["d2"] <= 900.0, t["d2"] <= 100.0
        qq = rec["ele_charges"][:, None] * lig["ele_charges"][None, :]
        inv = (np.float32(1.0) / d2.astype(np.float32)).astype(np.float64)
        e = np.clip(qq * inv, -dr.ELEC_MAX, dr.ELEC_MAX)
        broken = {"rcp": -(np.sum(e[cut]) * 332.0 / 4.0 + want[p]["vdw"]),
                  "cutoff": -(np.sum(t["e"][d2 < 900.0]) * 332.0 / 4.0 + want[p]["vdw"]),
                  "clamp": -(want[p]["elec"] * 332.0 / 4.0 + np.sum(np.minimum(t["k_raw"], 2.0)[cut_vdw]))}
        for what, energy in broken.items():
            # np.sum is not exact: allow it the order-of-sum share of the bound on top, and still be caught
            caught[what] += abs(energy - want[p]["energy"]) > 2.0 * want[p]["bound"]
    print("poses of 64 x 64 that catch each breakage:", caught)
    assert caught["rcp"] >= len(poses) // 2 and caught["cutoff"] >= 1 and caught["clamp"] >= 1
    assert abs(want[dr.ROW_900]["energy"]) > 0.0
