"""Energy decomposition on the GPU (ld_scorer_decompose; include/lightdock_hip.h "Energy decomposition").

The reference is a numpy restatement of the definition inside this file: poses by `orc.q_rotate` per atom, the terms of
every pair by the definition's formulas, elementwise, and the sequential sums as `np.cumsum(np.where(mask, t, 0.0),
axis=1)[:, -1]`.  cumsum is strictly sequential, so the restatement fixes the same bits as the kernels' definition:
per-atom sums, counts and flags are compared with np.array_equal -- a difference in the last bit is a finding about
contraction or order, never a reason for a tolerance.  Terms are also held against the oracle (`energy_ex_row`) and the
energy path."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, case_kwargs, case_positions
from dna_reference import IFACE2, N_POSES, posed, synthetic, synthetic_poses
from test_gpu_parity import REL_TOL, bm_err, rel_err

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def dfire_bin(d2):
    """DIST_TO_BINS[(sqrt(d2) * 2 - 1) as usize] - 1 (src/dfire.rs:49-53,336-337) for d2 <= 225: half-angstrom bins up to
    8 A, then one-angstrom bins; `as usize` saturates a negative d to 0; r = 15.0 gives bin 20, past the row."""
    d = np.sqrt(d2) * 2.0 - 1.0
    idx = np.maximum(d, 0.0).astype(np.int64)
    return np.where(idx < 3, 1, np.where(idx < 15, idx - 1, 14 + (idx - 15) // 2)) - 1, d


def seq_sum(t, mask, axis_owner):
    """Per owner the sequential sum of its masked terms in ascending partner index.  t, mask: (rec, lig)."""
    m = np.where(mask, t, 0.0)
    if axis_owner == 1:
        m = m.T
    return np.cumsum(m, axis=1)[:, -1]


def restate(orc, method, rec, lig, table, row, anm_rec=0, anm_lig=0):
    """One pose -> dict: per side sums (n, 2), pairs, flags; the terms; P and sum |t| per term (for the oracle bound)."""
    R = posed(orc, rec, row, False, row[7:7 + anm_rec])
    L = posed(orc, lig, row, True, row[7 + anm_rec:7 + anm_rec + anm_lig])
    dx = R[:, None, 0] - L[None, :, 0]
    dy = R[:, None, 1] - L[None, :, 1]
    dz = R[:, None, 2] - L[None, :, 2]
    d2 = dx * dx + dy * dy + dz * dz
    with np.errstate(all="ignore"):
        if method == "dfire":
            cut = d2 <= 225.0
            b, d = dfire_bin(np.where(cut, d2, 0.0))
            idx = rec["dfire_types"].astype(np.int64)[:, None] * 3380 + lig["dfire_types"].astype(np.int64)[None, :] * 20 + b
            terms = [(table[idx], cut)]
            count, iface = cut, cut & (d <= 3.9)
        else:
            cut = d2 <= 900.0
            e = rec["ele_charges"][:, None] * lig["ele_charges"][None, :] / d2
            e = np.where(e > 4.0 / 332.0, 4.0 / 332.0, e)
            e = np.where(e < -4.0 / 332.0, -4.0 / 332.0, e)
            vdw_energy = np.sqrt(rec["vdw_charges"][:, None] * lig["vdw_charges"][None, :])
            rr = rec["vdw_radii"][:, None] + lig["vdw_radii"][None, :]
            rr2 = rr * rr
            p6 = rr2 * (rr2 * rr2) / (d2 * d2 * d2)
            k = vdw_energy * (p6 * p6 - 2.0 * p6)
            k = np.where(k > 1.0, 1.0, k)
            terms = [(e, cut), (k, d2 <= 100.0)]
            count, iface = cut, d2 <= IFACE2
        out = {"P": [int(m.sum()) for _, m in terms], "abs": [float(np.abs(np.where(m, t, 0.0)).sum()) if np.all(np.isfinite(np.where(m, t, 0.0))) else np.nan for t, m in terms]}
        for side, key in ((0, "rec"), (1, "lig")):
            n = d2.shape[side]
            sums = np.zeros((n, 2))
            for c, (t, m) in enumerate(terms):
                sums[:, c] = seq_sum(t, m, side)
            out[key] = {"sums": sums, "pairs": count.sum(axis=1 - side).astype(np.uint32), "interface": iface.any(axis=1 - side).astype(np.uint32)}
        pair = [np.cumsum(out["rec"]["sums"][:, c])[-1] for c in range(2)]
        score = (pair[0] * 0.0157 - 4.7) * -1.0 if method == "dfire" else (pair[0] * 332.0 / 4.0 + pair[1]) * -1.0
        frac = []
        for key, mol in (("rec", rec), ("lig", lig)):
            offs, flags = mol.get("restraint_offsets"), out[key]["interface"]
            ng = 0 if offs is None else len(offs) - 1
            hit = sum(1 for g in range(ng) if flags[mol["restraint_atoms"][offs[g]:offs[g + 1]]].any())
            frac.append(hit / ng if ng else 0.0)
        beads = rec.get("membrane")
        membrane = float(out["rec"]["interface"][beads].sum()) / len(beads) if beads is not None and len(beads) else 0.0
        penalty = 999.0 * membrane if membrane > 0.0 else 0.0
        out["terms"] = dict(pair=pair, score=score, rec_restraints=frac[0], lig_restraints=frac[1], membrane=membrane,
                            energy=score + frac[0] * score + frac[1] * score - penalty, pairs=int(count.sum()),
                            rec_interface=int(out["rec"]["interface"].sum()), lig_interface=int(out["lig"]["interface"].sum()))
    return out


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def check_atoms(got, want, p, where):
    for key in ("rec", "lig"):
        assert same(got[key]["sums"][p], want[key]["sums"]), (where, p, key, "sums")
        assert np.array_equal(got[key]["pairs"][p], want[key]["pairs"]), (where, p, key, "pairs")
        assert np.array_equal(got[key]["interface"][p], want[key]["interface"]), (where, p, key, "interface")


def check_terms_exact(t, want, where):
    """The terms against the restatement: the same sequential sums, hence the same bits."""
    for k in ("score", "rec_restraints", "lig_restraints", "membrane", "energy"):
        assert same(t[k], want[k]), (where, k, t[k], want[k])
    assert same(t["pair"], want["pair"]), (where, "pair")
    for k in ("pairs", "rec_interface", "lig_interface"):
        assert int(t[k]) == want[k], (where, k)
    assert int(t["reserved"]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 1. synthetic molecules: the lane, workgroup and LDS-chunk edges; the cutoffs hit exactly; NaN
# ---------------------------------------------------------------------------------------------------------------------
PARTNER_CHUNK = 512     # kDecomposeChunk of csrc/kernels/decompose.hpp (tests/test_decompose_cpu.py holds the two together)
SHAPES = [(1, 1), (63, 65), (64, 64), (257, 255), (300, PARTNER_CHUNK + 1)]


@pytest.fixture(scope="module")
def molecules():
    """The molecules and poses of a shape, shared by the three methods."""
    cache = {}

    def get(shape):
        if shape not in cache:
            rec, lig = synthetic(shape[0], shape[1], 1000 * shape[0] + shape[1])
            poses = synthetic_poses(7)
            cache[shape] = (rec, lig, poses)
        return cache[shape]
    return get


@pytest.mark.parametrize("method", ["dfire", "dna", "pydock"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_per_atom_sums_counts_and_flags_are_the_restatements_bits(pkg, orc, table, molecules, shape, method):
    pkg.init(0)
    rec, lig, poses = molecules(shape)
    pick = (lambda m: {k: m[k] for k in ("coordinates", "dfire_types")}) if method == "dfire" else \
        (lambda m: {k: m[k] for k in ("coordinates", "ele_charges", "vdw_charges", "vdw_radii")})
    hip = pkg.Scorer.from_arrays(method, pick(rec), pick(lig), potential=table if method == "dfire" else None)
    assert hip.pose_len == 7 and poses.shape[1] == hip.pose_len + 3
    want = [restate(orc, "dfire" if method == "dfire" else "dna", rec, lig, table, row) for row in poses]
    for n in (1, 3, N_POSES):
        got = hip.decompose(poses[:n], atoms=True)
        assert got["rec"]["sums"].shape == (n, shape[0], 2) and got["lig"]["pairs"].shape == (n, shape[1])
        for p in range(n):
            check_atoms(got, want[p], p, (shape, method, n))
            check_terms_exact(got["terms"][p], want[p]["terms"], (shape, method, n, p))
    got = hip.decompose(poses, atoms=True)
    t = got["terms"]
    # pose 0: the pair of the two atoms 0 at d2 = 225 exactly counts (DFIRE reads bin 20, past the row); pose 1: nothing
    if method == "dfire":
        assert got["rec"]["pairs"][0, 0] >= 1 and got["lig"]["pairs"][0, 0] >= 1
        if shape == (1, 1):
            i = int(rec["dfire_types"][0]) * 3380 + int(lig["dfire_types"][0]) * 20 + 20
            assert t["pairs"][0] == 1 and t["pair"][0, 0] == table[i] and t["rec_interface"][0] == 0
            assert [int(v) for v in t["pairs"][3:6]] == [0, 1, 1] and [int(v) for v in t["rec_interface"][3:6]] == [0, 0, 0]
            assert t["rec_interface"][2] == 1 and t["lig_interface"][2] == 1      # d = -1 <= 3.9
        assert np.all(got["rec"]["sums"][..., 1] == 0.0) and np.all(t["pair"][:, 1] == 0.0)
    else:
        if shape == (1, 1):
            assert [int(v) for v in t["pairs"][[0, 3, 4, 5]]] == [1, 1, 1, 1]                     # 225, 900, 100, 15.21: all inside 900
            vdw = got["rec"]["sums"][:, 0, 1]
            assert vdw[0] == 0.0 and vdw[3] == 0.0 and vdw[4] != 0.0 and vdw[5] != 0.0          # van der Waals up to 100 inclusive
            assert [int(v) for v in t["rec_interface"][[0, 3, 4, 5]]] == [0, 0, 0, 1]            # interface at 3.9 * 3.9 inclusive
        # coincident atoms: NaN on both sides and in the energy, and nowhere it does not belong
        assert np.isnan(got["rec"]["sums"][2, 0, 1]) and np.isnan(got["lig"]["sums"][2, 0, 1])
        assert np.isnan(t["pair"][2, 1]) and np.isnan(t["score"][2]) and np.isnan(t["energy"][2])
        assert not np.isnan(got["rec"]["sums"][2, 0, 0]) and not np.isnan(got["rec"]["sums"][2, 1:]).any()
    for key in ("rec", "lig"):
        assert not got[key]["sums"][1].any() and not got[key]["pairs"][1].any() and not got[key]["interface"][1].any()
    assert t["pairs"][1] == 0 and t["pair"][1, 0] == 0.0 and t["energy"][1] == (4.7 if method == "dfire" else 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# the fixtures: restraints, beads, ANM
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(pkg, orc, table):
    pkg.init(0)
    cache = {}

    def get(name, method=None):
        key = (name, method)
        if key not in cache:
            m, rec, lig, kw = case_kwargs(name, orc, table)
            m = method or m
            hip, cpu = pkg.Scorer.from_pdb(m, rec, lig, **kw), orc.Scorer(m, rec, lig, **kw)
            mols = []
            for side, pdb, tag in ((0, rec, "rec"), (1, lig, "lig")):
                mol = cpu.model(side)
                if kw["use_anm"] and kw[tag + "_num_anm"] > 0:
                    mol["modes"] = np.asarray(kw[tag + "_nmodes"], dtype=np.float64).reshape(kw[tag + "_num_anm"], -1, 3)
                built = pkg.model_from_pdb(m, pdb)
                mol["residues"], mol["residue_of_atom"] = built["residues"], built["residue_of_atom"]
                mols.append(mol)
            anm = (kw["rec_num_anm"], kw["lig_num_anm"]) if kw["use_anm"] else (0, 0)
            cache[key] = dict(hip=hip, cpu=cpu, rec=mols[0], lig=mols[1], anm=anm, method="dfire" if m == "dfire" else "dna")
        return cache[key]
    return get


def fixture_poses(name, cases, orc):
    c = cases(name)
    poses = case_positions(name, orc)
    if name == "1ppe":
        return poses[:3]
    if name == "1k4c":     # the second pose puts ligand atom 0 onto a membrane bead
        row = poses[1].copy()
        row[3:7] = [1.0, 0.0, 0.0, 0.0]
        row[:3] = c["rec"]["coordinates"][c["rec"]["membrane"][0]] - c["lig"]["coordinates"][0]
        return np.stack([poses[0], row])
    if name == "2uuy":
        return poses[:2]
    return poses[:3]


@pytest.fixture(scope="module")
def decomposed(cases, orc, table):
    """Per fixture: the poses, the restatement of every pose (computed once, shared), one decompose() with atoms and one
    with residues."""
    cache = {}

    def get(name, method=None):
        key = (name, method)
        if key not in cache:
            c = cases(name, method)
            poses = fixture_poses(name, cases, orc)
            if method == "pydock":
                poses = poses[:1]
            want = [restate(orc, c["method"], c["rec"], c["lig"], table, row, *c["anm"]) for row in poses]
            atoms = c["hip"].decompose(poses, atoms=True)
            res = c["hip"].decompose(poses, rec_groups=c["rec"]["residue_of_atom"], lig_groups=c["lig"]["residue_of_atom"])
            cache[key] = dict(case=c, poses=poses, want=want, atoms=atoms, residues=res)
        return cache[key]
    return get


FIXTURES = [("1ppe", None), ("1k4c", None), ("2uuy", None), ("1azp", None), ("1azp", "pydock")]


@pytest.mark.parametrize("name,method", FIXTURES)
def test_fixture_atoms_are_the_restatements_bits(decomposed, name, method):
    d = decomposed(name, method)
    assert len(d["poses"]) == {"1ppe": 3, "1k4c": 2, "2uuy": 2, "1azp": 1 if method else 3}[name]
    for p, want in enumerate(d["want"]):
        check_atoms(d["atoms"], want, p, name)
        check_terms_exact(d["atoms"]["terms"][p], want["terms"], (name, p))
    assert np.array_equal(d["atoms"]["terms"], d["residues"]["terms"])


@pytest.mark.parametrize("name,method", FIXTURES)
def test_groups_are_the_sequential_sums_of_their_atoms(decomposed, name, method):
    """2. Residues from model_from_pdb, and a random non-contiguous map with an empty group and LD_GROUP_NONE atoms."""
    d = decomposed(name, method)
    c, poses = d["case"], d["poses"]
    rng = np.random.default_rng(5)
    n_random = 9
    maps = {}
    for key in ("rec", "lig"):
        n = len(c[key]["residue_of_atom"])
        m = rng.integers(0, n_random, n).astype(np.uint32)
        m[m == 4] = 5                                    # group 4 is empty
        m[rng.random(n) < 0.2] = 0xffffffff              # LD_GROUP_NONE
        m[-1] = n_random - 1
        maps[key] = m
    rnd = c["hip"].decompose(poses, rec_groups=maps["rec"], lig_groups=maps["lig"])
    for got, gmaps in ((d["residues"], {k: c[k]["residue_of_atom"] for k in ("rec", "lig")}), (rnd, maps)):
        for key in ("rec", "lig"):
            gmap = gmaps[key]
            n_groups = int(gmap[gmap != 0xffffffff].max()) + 1
            assert got[key]["sums"].shape == (len(poses), n_groups, 2)
            for p in range(len(poses)):
                a = d["atoms"][key]
                for g in range(n_groups):
                    idx = np.flatnonzero(gmap == g)      # ascending atom index
                    for col in range(2):
                        want = np.cumsum(np.concatenate([[0.0], a["sums"][p, idx, col]]))[-1]
                        assert same(got[key]["sums"][p, g, col], want), (name, key, p, g, col)
                    assert got[key]["pairs"][p, g] == a["pairs"][p, idx].sum() and got[key]["interface"][p, g] == a["interface"][p, idx].sum()
    assert not rnd["rec"]["sums"][:, 4].any() and not rnd["rec"]["pairs"][:, 4].any() and not rnd["lig"]["interface"][:, 4].any()


@pytest.mark.parametrize("name,method", FIXTURES)
def test_terms_against_the_oracle(decomposed, name, method):
    """3. Counts and fractions exact; energy within the suite's REL_TOL; pair[k] within 2 P 2^-53 sum |t|, the standard
    bound for two f64 sums of the same terms in different association (P terms: each sum errs by at most (P - 1) 2^-53
    sum |t| to first order)."""
    d = decomposed(name, method)
    cpu = d["case"]["cpu"]
    t = d["atoms"]["terms"]
    for p, row in enumerate(d["poses"]):
        energy, stats = cpu.energy_ex_row(row)
        want = d["want"][p]
        assert int(t["pairs"][p]) == int(stats[5]) and int(t["rec_interface"][p]) == int(stats[6]) and int(t["lig_interface"][p]) == int(stats[7])
        assert t["rec_restraints"][p] == stats[2] and t["lig_restraints"][p] == stats[3] and t["membrane"][p] == stats[4]
        assert rel_err(np.array([t["energy"][p]]), np.array([energy])) <= REL_TOL
        for k in range(1 if d["case"]["method"] == "dfire" else 2):
            bound = 2.0 * want["P"][k] * 2.0 ** -53 * want["abs"][k]
            print("%s pose %d pair[%d]: got %.17g oracle %.17g bound %.3g" % (name, p, k, t["pair"][p, k], stats[k], bound))
            assert abs(t["pair"][p, k] - stats[k]) <= bound
    if name == "1k4c":
        assert cpu.energy_ex_row(d["poses"][1])[1][4] > 0 and t["membrane"][1] > 0      # a bead at the interface
    if name == "1ppe":
        assert d["case"]["rec"]["restraint_offsets"].size == 2                           # the E.ILE.16 restraint
    if name == "1azp" and not method:
        assert d["case"]["rec"]["restraint_offsets"].size == 4 and d["case"]["lig"]["restraint_offsets"].size == 2


@pytest.mark.parametrize("name,method", FIXTURES)
def test_terms_against_the_energy_path(pkg, decomposed, name, method):
    """4. terms.energy against energy_batch of the same scorer; terms.pairs equals pair_counts of energy_batch_device."""
    torch = pytest.importorskip("torch")
    d = decomposed(name, method)
    hip, poses = d["case"]["hip"], d["poses"]
    t = d["atoms"]["terms"]
    err = bm_err if hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs" else rel_err
    assert err(t["energy"], hip.energy_batch(poses)) <= REL_TOL
    dev = torch.device("cuda:0")
    n = len(poses)
    d_poses = torch.from_numpy(np.ascontiguousarray(poses)).to(dev)
    d_out = torch.zeros(n, dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    hip.set_stream(torch.cuda.current_stream().cuda_stream)
    hip.energy_batch_device(n, d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), None, d_cnt.data_ptr())
    torch.cuda.synchronize()
    hip.set_stream(0)
    assert np.array_equal(d_cnt.cpu().numpy().astype(np.int64), t["pairs"].astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the same bits whatever the batch; refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_same_bits_whatever_the_batch_and_refusals(pkg, cases, orc):
    import ctypes as C
    c = cases("1ppe")      # the smallest fixture
    hip = c["hip"]
    info = hip.decompose_info()
    assert 1 <= info["slice"] <= 4096
    base = case_positions("1ppe", orc)[:8]
    n = info["slice"] + 1
    poses = np.full((n, 10), np.nan)
    poses[:, :7] = base[np.arange(n) % 8]
    rmap, lmap = c["rec"]["residue_of_atom"], c["lig"]["residue_of_atom"]
    got = hip.decompose(poses, rec_groups=rmap, lig_groups=lmap)
    assert hip.decompose_info()["last_kernel_ms"] > 0.0
    first = np.arange(n) % 8
    assert np.array_equal(got["terms"], got["terms"][first])
    for key in ("rec", "lig"):
        for out in ("sums", "pairs", "interface"):
            assert np.array_equal(got[key][out], got[key][out][first], equal_nan=True), (key, out)
    atoms = hip.decompose(poses[n - 9:], atoms=True)            # the per-atom rows across the end of a differently placed batch
    for k in range(8):
        one = hip.decompose(base[k:k + 1], rec_groups=rmap, lig_groups=lmap)
        one_atoms = hip.decompose(base[k:k + 1], atoms=True)
        assert np.array_equal(one["terms"][0], got["terms"][k])
        j = int(np.flatnonzero((np.arange(n - 9, n) % 8) == k)[0])
        for key in ("rec", "lig"):
            for out in ("sums", "pairs", "interface"):
                assert np.array_equal(one[key][out][0], got[key][out][k])
                assert np.array_equal(one_atoms[key][out][0], atoms[key][out][j])

    # refusals: LD_ERR_INVALID and every output as it was
    lib = pkg.load_library()
    nr, nl = hip.num_atoms(0), hip.num_atoms(1)
    few = np.ascontiguousarray(poses[:4])
    terms = np.zeros(4, dtype=pkg.ENERGY_TERMS)
    terms["energy"] = -77.0
    outs = {k: (np.full((4, 6, 2), -7.5), np.full((4, 6), 77, dtype=np.uint32), np.full((4, 6), 78, dtype=np.uint32)) for k in ("rec", "lig")}
    before = (terms.copy(), {k: [a.copy() for a in v] for k, v in outs.items()})

    def call(n_poses, stride, rec_map, rec_groups, lig_map, lig_groups):
        structs = []
        for key, gmap, ng in (("rec", rec_map, rec_groups), ("lig", lig_map, lig_groups)):
            g = pkg._GroupEnergies()
            g.group_of_atom, g.n_groups = (None if gmap is None else gmap.ctypes.data_as(C.c_void_p)), ng
            g.sums, g.pairs, g.interface_atoms = (a.ctypes.data_as(C.c_void_p) for a in outs[key])
            structs.append(g)
        return lib.ld_scorer_decompose(hip.handle, n_poses, few.ctypes.data_as(C.c_void_p), stride, terms.ctypes.data_as(C.c_void_p),
                                       C.byref(structs[0]), C.byref(structs[1]))

    small_r, small_l = (rmap % 6).astype(np.uint32), (lmap % 6).astype(np.uint32)
    assert nr == small_r.size and nl == small_l.size
    for args in ((4, 6, small_r, 6, small_l, 6),                         # stride < pose_len
                 (4, 10, small_r, 5, small_l, 6),                        # a receptor group id >= n_groups
                 (4, 10, small_r, 6, small_l, 5),                        # a ligand group id >= n_groups
                 (4, 10, small_r, 0, small_l, 6),                        # n_groups = 0 with a map
                 (2 ** 63, 10, small_r, 6, small_l, 6),                  # n x n_groups overflows (n x stride does too)
                 (2 ** 64 // 16 // nr + 1, 10, None, 0, small_l, 6)):    # n x n_atoms overflows under a NULL map, n x stride does not
        assert call(*args) == -1, args
        assert lib.ld_last_error()
        assert np.array_equal(terms, before[0])
        for k in ("rec", "lig"):
            for a, b in zip(outs[k], before[1][k]):
                assert np.array_equal(a, b)
    assert call(0, 10, small_r, 6, small_l, 6) == 0 and np.array_equal(terms, before[0])      # n = 0 touches nothing
    assert call(4, 10, small_r, 6, small_l, 6) == 0 and not np.array_equal(terms, before[0])  # and the scorer still serves
    assert np.array_equal(terms, hip.decompose(few)["terms"])


# ---------------------------------------------------------------------------------------------------------------------
# 6. the tool
# ---------------------------------------------------------------------------------------------------------------------
def test_decompose_tool_on_a_small_1czy_run(pkg, orc, table, tmp_path):
    """A 2-swarm, 10-step DFIRE run of 1czy with the synthetic table through the package's GSO and save_many; decompose.py
    on that run; both lists parse; per candidate the residues of a side add up to the score less its constant, and the
    energy is energy_batch's at the same pose."""
    czy = os.path.join(GOLDEN, "1czy")
    run = tmp_path / "run"
    os.makedirs(run / "data")
    for f in ("setup.json", "lightdock_1czy_protein.pdb", "lightdock_1czy_peptide.pdb", "rec_nm.npy", "lig_nm.npy"):
        shutil.copy(os.path.join(czy, f), run)
    pkg.synth.write_dcparams(str(run / "data" / "DCparams"), table)
    pkg.init(0)
    kw = dict(rec_active=["A.SER.467"], use_anm=True, rec_num_anm=10, lig_num_anm=10, rec_nmodes=orc.read_npy(os.path.join(czy, "rec_nm.npy")),
              lig_nmodes=orc.read_npy(os.path.join(czy, "lig_nm.npy")), potential=pkg.load_dcparams(str(run / "data" / "DCparams")))
    hip = pkg.Scorer.from_pdb("dfire", str(run / "lightdock_1czy_protein.pdb"), str(run / "lightdock_1czy_peptide.pdb"), **kw)
    pos = np.stack([orc.parse_positions(os.path.join(czy, "init", "initial_positions_%d.dat" % s)) for s in (0, 1)])
    gso = pkg.GSO(hip, pos, seeds=[324324, 324324])
    gso.run(10)
    for s in (0, 1):
        os.makedirs(run / ("swarm_%d" % s))
    gso.save_many([0, 1], 10, [str(run / "swarm_0"), str(run / "swarm_1")])

    script = os.path.join(os.path.dirname(pkg.__file__), "decompose.py")
    r = subprocess.run([sys.executable, script, "setup.json", "10", "dfire", "--swarms", "0-1", "--all", "--top", "12"], cwd=run,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "12 models decomposed" in r.stdout

    sys.path.insert(0, os.path.dirname(pkg.__file__))
    try:
        from analyse import read_gso
    finally:
        sys.path.pop(0)
    import importlib.util
    spec = importlib.util.spec_from_file_location("lightdock_rust_amd.decompose", script)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    head, rows = tool.parse_list((run / "decomposition" / "terms.list").read_text())
    rhead, rrows = tool.parse_list((run / "decomposition" / "residues.list").read_text())
    assert len(rows) == 12 and all(len(x) == len(head) for x in rows) and rrows and all(len(x) == len(rhead) for x in rrows)
    col = {h: k for k, h in enumerate(head)}
    scoring = [float(x[col["Scoring"]]) for x in rows]
    assert scoring == sorted(scoring, reverse=True)
    err = bm_err if hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs" else rel_err
    gso_poses = {s: read_gso(str(run / ("swarm_%d" % s) / "gso_10.out"))[0] for s in (0, 1)}
    for x in rows:
        s, g = int(x[0]), int(x[1])
        score, energy = float(x[col["Score"]]), float(x[col["Energy"]])
        for side in ("R", "L"):
            parts = [float(y[rhead.index("Energy")]) for y in rrows if (int(y[0]), int(y[1]), y[2]) == (s, g, side)]
            assert parts and abs(sum(parts) - (score - 4.7)) <= REL_TOL * max(abs(score - 4.7), 1e-9), (s, g, side)
        want = hip.energy_batch(gso_poses[s][g][None, :hip.pose_len])[0]
        assert err(np.array([energy]), np.array([want])) <= REL_TOL
