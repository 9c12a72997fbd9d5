"""A plain restatement of the DNA / PYDOCK pose energy with an exact sum and a derived error bound (the DNA
pair body).  A helper module, not a test: tests/test_dna_reference_cpu.py holds it to the oracle, and
tests/test_gpu_dna_pairs.py holds pose_energy_pairs<1, *> to it.

Geometry is `posed`: the oracle's own quaternion rotation per atom, + t, then ANM in ascending mode order, and
d2 = dx*dx + dy*dy + dz*dz with dx = R - L in f64, so every cutoff decision is the kernel's decision bit for bit.  The
terms are f64 by the reference's formulas (src/dna.rs:471-512); the sums are math.fsum, which is exact.

The bound is the allowed |kernel - reference| of one pose, from the reference's terms alone (delta = 2^-46, u = 2^-53):
  reciprocal   delta * sum|e| * 332/4  +  sum over d2 <= 100 with unclamped k <= 2 of 6 delta sqrt(er el) (p6^2 + p6)
  order        S u (sum|e| * 332/4 + sum|k|),  S = n_rec * ceil(n_lig / 64) + n_chunks + 16
  tail         (reciprocal + order) (1 + fr + fl)  +  8 u |energy|
delta is from documentation: v_rcp_f64 is good to about 2^-24, one Newton step squares that to 2^-48, its two fma
roundings and the product's rounding keep the term below 2^-47, delta is twice that.  inv^3 carries three reciprocal
errors into p6 and p6^2 doubles them; a pair whose unclamped k exceeds 2 cannot be brought under the clamp at 1 by a
relative error of that size.  S limits the additions any one value passes through: a lane's private chain, the two
trees and the finish fold."""
import math

import numpy as np

U = 2.0 ** -53
DELTA = 2.0 ** -46
IFACE2 = 3.9 * 3.9          # INTERFACE_CUTOFF2, src/constants.rs:15
ELEC_MAX = 4.0 / 332.0      # src/dna.rs:15-25
DEFAULT_CHUNK = 256         # AllPairsPath's receptor chunk for DNA when LIGHTDOCK_CHUNK_ATOMS is not set


# ---------------------------------------------------------------------------------------------------------------------
# geometry and synthetic inputs (shared with tests/test_gpu_decompose.py)
# ---------------------------------------------------------------------------------------------------------------------
def posed(orc, mol, row, ligand, ext):
    """One molecule at one pose: q v q^-1 + t for the ligand, then ANM in ascending mode order (src/dfire.rs:282-320)."""
    xyz = np.array(mol["coordinates"], dtype=np.float64).reshape(-1, 3)
    if ligand:
        xyz = np.stack([orc.q_rotate(row[3:7], v) for v in xyz]) + row[:3]
    modes = mol.get("modes")
    if modes is not None:
        xyz = xyz.copy()
        for k in range(modes.shape[0]):
            xyz += modes[k] * ext[k]
    return xyz


N_POSES = 37


def synthetic(n_rec, n_lig, seed):
    rng = np.random.default_rng(seed)

    def mol(n):
        xyz = rng.random((n, 3)) * 30.0
        xyz[0] = 0.0        # atom 0 of both molecules at the origin: a pose's translation IS their distance vector
        return {"coordinates": xyz, "dfire_types": rng.integers(0, 168, n).astype(np.uint32), "ele_charges": rng.random(n) - 0.5,
                "vdw_charges": 0.01 + 0.2 * rng.random(n), "vdw_radii": 1.0 + rng.random(n)}
    return mol(n_rec), mol(n_lig)


def synthetic_poses(seed):
    """37 rows of pose_len + 3 columns.  0: d2 = 225 exactly between the two atoms 0 (identity rotation); 1: 500 A away;
    2: the two atoms 0 coincide (DNA: NaN); 3, 4, 5: d2 = 900, 100 and 3.9 * 3.9 exactly; the rest random, quaternions
    not normalised."""
    rng = np.random.default_rng(seed)
    poses = np.full((N_POSES, 10), np.nan)
    poses[:, :3] = rng.random((N_POSES, 3)) * 20.0 - 10.0
    poses[:, 3:7] = rng.random((N_POSES, 4)) - 0.5
    for p, t in enumerate([(9.0, 12.0, 0.0), (500.0, 0.0, 0.0), (0.0, 0.0, 0.0), (18.0, 24.0, 0.0), (6.0, 8.0, 0.0), (3.9, 0.0, 0.0)]):
        poses[p, :7] = t + (1.0, 0.0, 0.0, 0.0)
    return poses


# ---------------------------------------------------------------------------------------------------------------------
# the shapes and poses of tests/test_gpu_dna_pairs.py
# ---------------------------------------------------------------------------------------------------------------------
# rows of dna_poses(): the six special rows of synthetic_poses, then the two just-outside rows, then its random rows
ROW_225, ROW_FAR, ROW_COINCIDENT, ROW_900, ROW_100, ROW_IFACE, ROW_OUTSIDE_900, ROW_OUTSIDE_100 = range(8)
N_SPECIAL = 8
N_ROWS_LARGE = 14       # shapes with more than 513 atoms on a side take the first 14 rows: all special rows and 6 random ones

# (n_rec, n_lig, LIGHTDOCK_CHUNK_ATOMS or None, the receptor chunks that gives): what each reaches is in the GPU test
SHAPES = [(1, 1, None, 1), (3, 65, None, 1), (64, 64, None, 1), (255, 256, None, 1), (256, 257, None, 1), (257, 63, None, 2),
          (513, 960, None, 3), (448, 64, 64, 7), (512, 65, 64, 8), (513, 130, 64, 9), (1025, 1025, 64, 17)]


def shape_id(shape):
    return "%dx%d" % shape[:2] + ("" if shape[2] is None else "-chunk%d" % shape[2])


def dna_poses():
    """synthetic_poses(7) with two rows put in after its six special ones: the atoms 0 at d2 = 900 + 2^-40 and at
    100 + 2^-40 (both sums are exact in f64), just outside the two cutoffs.  39 rows."""
    base = synthetic_poses(7)
    extra = np.full((2, base.shape[1]), np.nan)
    extra[0, :7] = (18.0, 24.0, 2.0 ** -20, 1.0, 0.0, 0.0, 0.0)
    extra[1, :7] = (6.0, 8.0, 2.0 ** -20, 1.0, 0.0, 0.0, 0.0)
    return np.concatenate([base[:6], extra, base[6:]])


def shape_molecules(shape):
    return synthetic(shape[0], shape[1], 1000 * shape[0] + shape[1])


def shape_poses(shape):
    poses = dna_poses()
    return poses if max(shape[:2]) <= 513 else poses[:N_ROWS_LARGE]


_shape_cache = {}


def shape_reference(orc, shape):
    """(rec, lig, poses, [dna_reference of every pose]) of one row of SHAPES: computed once, shared, never changed."""
    if shape not in _shape_cache:
        rec, lig = shape_molecules(shape)
        poses = shape_poses(shape)
        _shape_cache[shape] = (rec, lig, poses, [dna_reference(orc, rec, lig, row, n_chunks=shape[3]) for row in poses])
    return _shape_cache[shape]


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def dna_reference(orc, rec, lig, row, anm_rec=0, anm_lig=0, n_chunks=None, keep_terms=False):
    """One pose of ld_molecule-shaped dicts (optional keys: modes (k, n, 3), membrane, restraint_offsets,
    restraint_atoms) -> dict: elec, vdw, score, energy, pairs, rec_interface / lig_interface (flag per atom), nan, bound,
    and what the conditions on a test's inputs need.  n_chunks: the receptor chunks of the scorer under test (default:
    what the scorer takes when LIGHTDOCK_CHUNK_ATOMS is not set)."""
    R = posed(orc, rec, row, False, row[7:7 + anm_rec])
    L = posed(orc, lig, row, True, row[7 + anm_rec:7 + anm_rec + anm_lig])
    n_rec, n_lig = R.shape[0], L.shape[0]
    if n_chunks is None:
        n_chunks = -(-n_rec // DEFAULT_CHUNK)
    dx = R[:, None, 0] - L[None, :, 0]
    dy = R[:, None, 1] - L[None, :, 1]
    dz = R[:, None, 2] - L[None, :, 2]
    d2 = dx * dx + dy * dy + dz * dz
    cut, cut_vdw, iface = d2 <= 900.0, d2 <= 100.0, d2 <= IFACE2
    with np.errstate(all="ignore"):
        e_raw = (rec["ele_charges"][:, None] * lig["ele_charges"][None, :]) / d2
        e = np.where(e_raw > ELEC_MAX, ELEC_MAX, e_raw)
        e = np.where(e < -ELEC_MAX, -ELEC_MAX, e)
        depth = np.sqrt(rec["vdw_charges"][:, None] * lig["vdw_charges"][None, :])
        rr = rec["vdw_radii"][:, None] + lig["vdw_radii"][None, :]
        rr2 = rr * rr
        p6 = rr2 * (rr2 * rr2) / (d2 * d2 * d2)
        k_raw = depth * (p6 * p6 - 2.0 * p6)
        k = np.where(k_raw > 1.0, 1.0, k_raw)
        e_in, k_in = e[cut], k[cut_vdw]
        nan = bool(not np.all(np.isfinite(e_in)) or not np.all(np.isfinite(k_in)))
        elec = float(np.sum(e_in)) if nan else math.fsum(e_in)
        vdw = float(np.sum(k_in)) if nan else math.fsum(k_in)
        score = -(elec * 332.0 / 4.0 + vdw)

        # the tail, src/scoring.rs:21-47
        flags = (iface.any(axis=1), iface.any(axis=0))
        frac = []
        for mol, f in ((rec, flags[0]), (lig, flags[1])):
            offs = mol.get("restraint_offsets")
            ng = 0 if offs is None else len(offs) - 1
            hit = sum(1 for g in range(ng) if f[np.asarray(mol["restraint_atoms"][offs[g]:offs[g + 1]], dtype=np.int64)].any())
            frac.append(hit / ng if ng else 0.0)
        beads = rec.get("membrane")
        membrane = float(flags[0][np.asarray(beads, dtype=np.int64)].sum()) / len(beads) if beads is not None and len(beads) else 0.0
        penalty = 999.0 * membrane if membrane > 0.0 else 0.0
        energy = score + frac[0] * score + frac[1] * score - penalty

        abs_e = math.fsum(np.abs(e_in)) * 332.0 / 4.0 if not nan else np.nan
        abs_k = math.fsum(np.abs(k_in)) if not nan else np.nan
        soft = cut_vdw & (k_raw <= 2.0)
        rcp_vdw = math.fsum((6.0 * DELTA * depth * (p6 * p6 + p6))[soft]) if not nan else np.nan
        steps = n_rec * -(-n_lig // 64) + n_chunks + 16
        bound = (DELTA * abs_e + rcp_vdw + steps * U * (abs_e + abs_k)) * (1.0 + frac[0] + frac[1]) + 8.0 * U * abs(energy)

    out = dict(elec=elec, vdw=vdw, score=score, energy=energy, pairs=int(cut.sum()), rec_interface=flags[0], lig_interface=flags[1],
               nan=nan, bound=float(bound), rec_restraints=frac[0], lig_restraints=frac[1], membrane=membrane,
               P=(int(cut.sum()), int(cut_vdw.sum())), abs_terms=(abs_e, abs_k),
               seen=dict(e_high=int((cut & (e_raw > ELEC_MAX)).sum()), e_low=int((cut & (e_raw < -ELEC_MAX)).sum()),
                         k_clamped=int((cut_vdw & (k_raw > 1.0)).sum()), k_negative=int((cut_vdw & (k_raw < 0.0)).sum()),
                         between=int((cut & ~cut_vdw).sum()), beyond=int((~cut).sum()), interface=int(iface.sum())),
               near_cutoff=np.abs(e[(d2 > 800.0) & cut]) * 332.0 / 4.0)
    if keep_terms:
        out["terms"] = dict(d2=d2, e_raw=e_raw, e=e, k_raw=k_raw, k=k, depth=depth, p6=p6)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the tail and ANM cases of tests/test_gpu_dna_pairs.py
# ---------------------------------------------------------------------------------------------------------------------
TAIL_SHAPE = (257, 130, None, 2)
ANM_SHAPES = [(65, 63, None, 1), (257, 130, None, 2)]
ANM_MODES = [(3, 0), (0, 3), (1, 2)]
N_ROWS_ANM = 14

_case_cache = {}


def tail_case(orc):
    """257 x 130 with a tail: the receptor has two restraint groups (one holds atom 0, one is the four atoms nearest the
    far corner of the box) and five membrane atoms, atom 1 among them; the ligand has one restraint group with its last
    atom, which sits in the padded ligand group.  Poses: the first 14 rows of dna_poses() and three by hand (identity
    rotation): the ligand's last atom 1 A from a far-corner atom, the two molecules almost on top of each other, and
    ligand atom 0 1 A from the membrane atom 1.  -> (rec, lig, poses, references)."""
    if "tail" not in _case_cache:
        rec, lig = shape_molecules(TAIL_SHAPE)
        xyz = rec["coordinates"]
        far = np.argsort(-xyz.sum(axis=1))[:4]
        rec["restraint_offsets"] = np.array([0, 3, 7], dtype=np.uint32)
        rec["restraint_atoms"] = np.concatenate([[0, 100, 200], far]).astype(np.uint32)
        rec["membrane"] = np.array([1, 50, 120, 190, 256], dtype=np.uint32)
        n_lig = TAIL_SHAPE[1]
        lig["restraint_offsets"] = np.array([0, 2], dtype=np.uint32)
        lig["restraint_atoms"] = np.array([5, n_lig - 1], dtype=np.uint32)
        hand = np.full((3, 10), np.nan)
        hand[:, 3:7] = (1.0, 0.0, 0.0, 0.0)
        hand[0, :3] = xyz[far[0]] - lig["coordinates"][n_lig - 1] + (1.0, 0.0, 0.0)
        hand[1, :3] = (0.5, 0.5, 0.5)
        hand[2, :3] = xyz[1] - lig["coordinates"][0] + (1.0, 0.0, 0.0)
        poses = np.concatenate([dna_poses()[:N_ROWS_LARGE], hand])
        _case_cache["tail"] = (rec, lig, poses, [dna_reference(orc, rec, lig, row, n_chunks=TAIL_SHAPE[3]) for row in poses])
    return _case_cache["tail"]


def anm_case(orc, shape, k_rec, k_lig):
    """Modes normal * 0.4 on the sides that have some, extents normal * 2 in the pose's columns 7.. (receptor's first); the
    first 14 rows of dna_poses().  The molecule dicts carry `modes` (k, n, 3) for the restatement and `nmodes`, `num_anm`
    for Scorer.from_arrays.  -> (rec, lig, poses, references)."""
    key = (shape, k_rec, k_lig)
    if key not in _case_cache:
        rec, lig = shape_molecules(shape)
        rng = np.random.default_rng(100 * k_rec + k_lig)
        for mol, k in ((rec, k_rec), (lig, k_lig)):
            if k:
                mol["modes"] = rng.normal(size=(k, len(mol["coordinates"]), 3)) * 0.4
                mol["nmodes"], mol["num_anm"] = mol["modes"].ravel(), k
        poses = dna_poses()[:N_ROWS_ANM].copy()
        poses[:, 7:7 + k_rec + k_lig] = rng.normal(size=(len(poses), k_rec + k_lig)) * 2.0
        _case_cache[key] = (rec, lig, poses, [dna_reference(orc, rec, lig, row, k_rec, k_lig, n_chunks=shape[3]) for row in poses])
    return _case_cache[key]
