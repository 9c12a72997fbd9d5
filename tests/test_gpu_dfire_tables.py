"""DFIRE parity over POTENTIALS (run with -m gpu on an MI355X): every route to the DFIRE sum -- block-major `dfire_bm_pairs`,
pose-major `dfire_packed_pairs`, the all-pairs kernel -- on tables that vary what the block-major path's 64-bit fixed point
depends on: the scale exponent e (2^e >= the table's largest |value|), the extra bits x a crowded receptor takes off the
scale, the size and sign of a 32-pair half-sum under the marker field, and the tables the path declines.

The references are EXACT, so the tolerance is a count of roundings and not an empirical allowance:

1. Dyadic tables.  Every value is an integer multiple of 2^-g and pairs * max|v| * 2^g < 2^53 (asserted per pose): the
   oracle's f64 sum is exact in any order, the fixed-point rounding rint(v * 2^(44 - e - x)) is exact for g <= 44 - e - x, so
   every route owes the same raw sum bit for bit.  tests/test_dfire_tables_cpu.py proves the premise on the CPU: the oracle's
   stats[0] equals an integer restatement on the very poses used here.
2. Arbitrary tables (the stock synthetic one, a non-dyadic one at |v| <= 1000).  The block-major path's SPECIFIED result is
   exact too: sum of llrint(v * scale) over the in-cutoff pairs, divided by scale.  Python integers over the restatement's
   (type, type, bin) of every pair give that sum; poses on which the restatement and the oracle could disagree about a pair
   (a knife-edge distance: matrix posing here, quaternion product there) are left out by two guards, at most 2 % of a case.

What remains between the device and the host is the tail of src/dfire.rs:347-361, `TAIL_ROUNDINGS` roundings of intermediates
no larger than M = 3 max(|raw| 0.0157, 4.7) + 999: the energies are held to TAIL_ROUNDINGS * spacing(M).  The in-cutoff pair
counts are held to equality, the route to its name.

The table generators and the case builders live here; the CPU file imports them.
"""
import contextlib
import os

import numpy as np
import pytest

from conftest import case_kwargs, case_positions
from test_gpu_parity import REL_TOL, _RES_ATOMS, _random_molecule, _write_pdb, rel_err

pytestmark = pytest.mark.gpu

TABLE_LEN = 169 * 169 * 20
ROW = 169 * 20
# The tail, src/dfire.rs:347-361 as oracle/ld_oracle.c and pose_energy_finish evaluate it -- roundings, counted in the code:
# raw * 0.0157 (1), - 4.7 (2) [* -1.0 is exact], perc_rec * score (3), score + that (4), perc_lig * score (5), + that (6),
# 999.0 * intersection (7), - penalty (8).  The device may fuse a product into the add that follows (fewer roundings, other
# bits); the restraint and bead fractions are one correctly rounded division of the same integers on both sides.
TAIL_ROUNDINGS = 8
MAX_LEFT_OUT = 0.02          # share of a case's poses the knife-edge guards may leave out

BM, PACKED, ALLPAIRS = "dfire_bm_pairs", "dfire_packed_pairs", "pose_energy_pairs<0"
ROUTES = [({}, BM), ({"LIGHTDOCK_DFIRE_KERNEL": "packed"}, PACKED), ({"LIGHTDOCK_DFIRE_KERNEL": "allpairs"}, ALLPAIRS)]
ROUTE_IDS = ["bm", "packed", "allpairs"]

# (vmax, g): values are multiples of 2^-g in [-vmax, vmax]; the scale the block-major path owes is 2^(44 - e)
LADDER = [(2.0 ** -30, 44, 0), (1.0, 20, 0), (1.0 + 2.0 ** -20, 20, 1), (10.0, 20, 4), (16.0, 20, 4), (16.0 + 2.0 ** -20, 20, 5),
          (1024.0, 20, 10)]
LADDER_IDS = ["2^-30", "1", "1+2^-20", "10", "16", "16+2^-20", "1024"]
FIXTURE_POSES = {"1ppe": 24, "1k4c": 8, "2uuy": 10}


# ---- the integer restatement ---------------------------------------------------------------------------------------

_DIST_TO_BINS = np.array([1, 1, 1] + [i - 1 for i in range(3, 15)] + [14 + (i - 15) // 2 for i in range(15, 49)] + [31, 32])   # src/dfire.rs:49-53


def restate_pose(mr, ml, pose, rec_modes=None, lig_modes=None):
    """The flat table index ti * 3380 + tj * 20 + bin of every in-cutoff pair of one pose (src/dfire.rs:265-345 in numpy, the
    restatement of tests/test_oracle_scoring.py with normal modes added): the ligand posed by a rotation MATRIX, which the
    reference does by a quaternion product -- a pair at a knife-edge distance may land elsewhere, hence the guards."""
    k_rec = 0 if rec_modes is None else len(rec_modes)
    k_lig = 0 if lig_modes is None else len(lig_modes)
    t = pose[:3]
    w, x, y, z = pose[3:7]
    n2 = w * w + x * x + y * y + z * z
    R = np.array([[w*w+x*x-y*y-z*z, 2*(x*y-w*z), 2*(x*z+w*y)],
                  [2*(x*y+w*z), w*w-x*x+y*y-z*z, 2*(y*z-w*x)],
                  [2*(x*z-w*y), 2*(y*z+w*x), w*w-x*x-y*y+z*z]]) / n2
    lc = ml["coordinates"] @ R.T + t
    if k_lig:
        lc = lc + np.tensordot(pose[7 + k_rec:7 + k_rec + k_lig], lig_modes, 1)
    rc = mr["coordinates"]
    if k_rec:
        rc = rc + np.tensordot(pose[7:7 + k_rec], rec_modes, 1)
    rt, lt = mr["dfire_types"].astype(np.int64), ml["dfire_types"].astype(np.int64)
    out = []
    for lo in range(0, len(rc), 512):                       # (in slabs: 1k4c is 11 M pairs a pose)
        d2 = ((rc[lo:lo + 512, None, :] - lc[None, :, :]) ** 2).sum(-1)
        i, j = np.nonzero(d2 <= 225.0)
        d = np.sqrt(d2[i, j]) * 2.0 - 1.0
        bins = _DIST_TO_BINS[np.maximum(d, 0.0).astype(np.int64)] - 1
        out.append(rt[lo + i] * ROW + lt[j] * 20 + bins)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def isum(values):
    """Sum of an int64 array as a Python integer, whatever its size."""
    if len(values) == 0:
        return 0
    if len(values) * int(np.abs(values).max()) < 2 ** 62:
        return int(values.sum())
    return int(values.astype(object).sum())


def dyadic_ints(table, g):
    """table * 2^g as int64; asserts that every value IS a multiple of 2^-g."""
    ints = np.rint(np.ldexp(table, g)).astype(np.int64)
    assert np.array_equal(np.ldexp(ints.astype(np.float64), -g), table), "not a dyadic table at g = %d" % g
    return ints


def fits_53_bits(s):
    s = abs(int(s))
    return s == 0 or (s >> ((s & -s).bit_length() - 1)).bit_length() <= 53


def tail(raw, stats):
    """src/dfire.rs:347-361 on the host in f64, operation by operation the oracle's; stats: the oracle's (fractions and bead share)."""
    score = (float(raw) * 0.0157 - 4.7) * -1.0
    penalty = 999.0 * float(stats[4]) if stats[4] > 0.0 else 0.0
    return score + float(stats[2]) * score + float(stats[3]) * score - penalty


def tail_bound(raw):
    """M of the module docstring."""
    return 3.0 * np.maximum(np.abs(raw) * 0.0157, 4.7) + 999.0


ULPS = {}      # table class -> the largest |got - want| / spacing(M) seen in this session (printed per test)


def hold_exact(label, klass, got, want, raw, extra=0.0):
    """|got - want| <= TAIL_ROUNDINGS * spacing(M) (+ extra, where the reference says so)."""
    got, want, raw = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(raw, dtype=np.float64)
    unit = np.spacing(tail_bound(raw))
    ulps = np.abs(got - want) / unit
    worst = float(np.max(ulps)) if len(ulps) else 0.0
    ULPS[klass] = max(ULPS.get(klass, 0.0), worst)
    print("TABLES %-10s %-48s worst |got - want| = %.3f spacing(M); class so far %.3f" % (klass, label, worst, ULPS[klass]))
    bad = np.flatnonzero(~(np.abs(got - want) <= TAIL_ROUNDINGS * unit + extra))
    assert bad.size == 0, (label, bad[:8], got[bad[:8]], want[bad[:8]], ulps[bad[:8]])


# ---- cases: molecules, restraints, modes, poses ----------------------------------------------------------------------

class Case:
    """One complex and its poses; `kw` are the constructor arguments of both scorers, the potential excepted."""

    def __init__(self, label, rec, lig, kw, poses, rec_modes=None, lig_modes=None):
        self.label, self.rec, self.lig, self.kw, self.poses = label, rec, lig, kw, np.ascontiguousarray(poses, dtype=np.float64)
        self.rec_modes, self.lig_modes = rec_modes, lig_modes
        self._idx = None

    def cpu(self, orc, table):
        return orc.Scorer("dfire", self.rec, self.lig, potential=table, **self.kw)

    def hip(self, pkg, table, env=None):
        with _environment(env or {}):
            return pkg.Scorer.from_pdb("dfire", self.rec, self.lig, potential=table, **self.kw)

    def idx(self, orc):
        """restate_pose of every pose (kept: the tables of a case share them)."""
        if self._idx is None:
            s = self.cpu(orc, np.zeros(TABLE_LEN))
            mr, ml = s.model(0), s.model(1)
            rm = None if self.rec_modes is None else np.asarray(self.rec_modes, dtype=np.float64).ravel()[:self.kw["rec_num_anm"] * len(mr["coordinates"]) * 3].reshape(-1, len(mr["coordinates"]), 3)
            lm = None if self.lig_modes is None else np.asarray(self.lig_modes, dtype=np.float64).ravel()[:self.kw["lig_num_anm"] * len(ml["coordinates"]) * 3].reshape(-1, len(ml["coordinates"]), 3)
            self.n_rec, self.n_lig = len(mr["coordinates"]), len(ml["coordinates"])
            self._idx = [restate_pose(mr, ml, p, rm, lm) for p in self.poses]
        return self._idx

    def used(self, orc):
        """Table entries that pose 0 reads, most read first (where a generator plants its extreme values)."""
        u, n = np.unique(self.idx(orc)[0], return_counts=True)
        return u[np.argsort(-n, kind="stable")]


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_FIXTURES = {}


def fixture_case(name, orc):
    """1ppe (a restraint), 1k4c (membrane beads), 2uuy (10 + 10 normal modes) on the reference's starting poses."""
    if name not in _FIXTURES:
        _, rec, lig, kw = case_kwargs(name, orc, None)
        kw.pop("potential")
        _FIXTURES[name] = Case(name, rec, lig, kw, case_positions(name, orc)[:FIXTURE_POSES[name]], kw.get("rec_nmodes"), kw.get("lig_nmodes"))
    return _FIXTURES[name]


def random_rigid_case(tmp_path, n_rec, n_lig, restraints):
    """The molecules and poses of test_gpu_parity.py::test_random_molecules_match_oracle (same seed, same draws): its four
    OVERLAPPING poses -- whole 8 x 8 blocks inside the cutoff -- and four of the others."""
    rng = np.random.default_rng(1000 * n_rec + n_lig)
    rec, lig = str(tmp_path / "rec.pdb"), str(tmp_path / "lig.pdb")
    rec_atoms = _random_molecule(rng, n_rec, 28.0, "A", with_beads=3 if n_rec >= 64 else 0)
    lig_atoms = _random_molecule(rng, n_lig, 18.0, "B")
    _write_pdb(rec, rec_atoms)
    _write_pdb(lig, lig_atoms)
    poses = np.zeros((24, 7))
    poses[:, :3] = rng.uniform(-22, 22, (24, 3))
    poses[:4, :3] = rng.uniform(-2, 2, (4, 3))
    q = rng.normal(size=(24, 4))
    poses[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (24, 1))
    kw = dict(rec_active=["A.%s.%d" % (rec_atoms[0][1], rec_atoms[0][3])], lig_active=["B.%s.%d" % (lig_atoms[-1][1], lig_atoms[-1][3])]) if restraints else {}
    return Case("random %dx%d%s" % (n_rec, n_lig, " restrained" if restraints else ""), rec, lig, kw, poses[:8])


def random_anm_case(tmp_path, n_rec, n_lig, k_rec, k_lig, restraints):
    """The molecules, modes and poses of test_gpu_parity.py::test_random_molecules_with_normal_modes_match_oracle: a tenth of
    the poses WILD (everything through the exact path), four overlapping."""
    rng = np.random.default_rng(7000 * n_rec + n_lig)
    rec, lig = str(tmp_path / "rec.pdb"), str(tmp_path / "lig.pdb")
    rec_atoms = _random_molecule(rng, n_rec, 28.0, "A", with_beads=3 if n_rec >= 64 else 0)
    lig_atoms = _random_molecule(rng, n_lig, 18.0, "B")
    _write_pdb(rec, rec_atoms)
    _write_pdb(lig, lig_atoms)
    n = 30
    poses = np.zeros((n, 7 + k_rec + k_lig))
    poses[:, :3] = rng.uniform(-22, 22, (n, 3))
    poses[:4, :3] = rng.uniform(-2, 2, (4, 3))
    q = rng.normal(size=(n, 4))
    poses[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))
    poses[:, 7:] = rng.normal(size=(n, k_rec + k_lig)) * 2.0
    poses[::10, 7:] *= 40.0
    kw = dict(use_anm=True, rec_num_anm=k_rec, lig_num_anm=k_lig,
              rec_nmodes=(rng.normal(size=(k_rec, len(rec_atoms), 3)) * 0.4).ravel() if k_rec else None,
              lig_nmodes=(rng.normal(size=(k_lig, len(lig_atoms), 3)) * 0.4).ravel() if k_lig else None)
    if restraints:
        kw.update(rec_active=["A.%s.%d" % (rec_atoms[0][1], rec_atoms[0][3])], lig_active=["B.%s.%d" % (lig_atoms[-1][1], lig_atoms[-1][3])])
    return Case("random anm %dx%d (%d+%d)%s" % (n_rec, n_lig, k_rec, k_lig, " restrained" if restraints else ""), rec, lig, kw, poses,
                kw["rec_nmodes"], kw["lig_nmodes"])


def _residue_atoms(rng, xyz, chain):
    atoms, seq, k = [], 1, 0
    names = sorted(_RES_ATOMS)
    while k < len(xyz):
        res = names[int(rng.integers(len(names)))]
        for a in _RES_ATOMS[res]:
            if k < len(xyz):
                atoms.append((a, res, chain, seq, xyz[k][0], xyz[k][1], xyz[k][2]))
                k += 1
        seq += 1
    return atoms


def ball_xyz(n, seed):
    """n distinct points, rounded to 0.001, at random in a ball of radius 8 A."""
    rng = np.random.default_rng(seed)
    seen, pts = set(), []
    while len(pts) < n:
        for p in np.round(rng.uniform(-8.0, 8.0, (n, 3)), 3):
            key = tuple(p)
            if p @ p <= 64.0 and key not in seen and len(pts) < n:
                seen.add(key)
                pts.append(p)
    return np.array(pts)


def ball_case(tmp_path, n_rec, n_lig, restraints=False):
    """A receptor of n_rec ordinary residue atoms in a ball of radius 8 A against a ligand in a 3 A cube, posed by the identity
    and by small moves: EVERY pair is inside the cutoff (8 + 3 sqrt(3) / 2 + 1.8 < 15; asserted from the oracle's count by the
    tests), so one ligand tile reaches all n_rec atoms -- the count that takes bits off the block-major scale from 8192 on."""
    rng = np.random.default_rng(50000 + 7 * n_rec + n_lig)
    rec, lig = str(tmp_path / "ball.pdb"), str(tmp_path / "cube.pdb")
    rec_atoms = _residue_atoms(rng, ball_xyz(n_rec, n_rec), "A")
    lig_atoms = _random_molecule(rng, n_lig, 3.0, "B")
    _write_pdb(rec, rec_atoms)
    _write_pdb(lig, lig_atoms)
    poses = np.zeros((6, 7))
    poses[:, 3] = 1.0
    poses[1:, :3] = rng.uniform(-1.0, 1.0, (5, 3))
    q = rng.normal(size=(3, 4))
    poses[3:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    kw = {}
    if restraints:   # several residues a side: their atoms' blocks are tracked, i.e. carry markers in bins 0 and 1 as well
        kw = dict(rec_active=sorted({"A.%s.%d" % (a[1], a[3]) for a in rec_atoms[::max(1, n_rec // 12)]}),
                  lig_active=sorted({"B.%s.%d" % (a[1], a[3]) for a in lig_atoms[::max(1, n_lig // 4)]}))
    return Case("ball %dx%d%s" % (n_rec, n_lig, " restrained" if restraints else ""), rec, lig, kw, poses)


# ---- tables (seeded; dyadic unless the name says otherwise) --------------------------------------------------------------

def ladder_table(vmax, g, used, seed=0):
    """Random multiples of 2^-g in [-vmax, vmax], +vmax and -vmax themselves in two entries that the complex reads."""
    top = int(round(vmax * 2.0 ** g))
    assert top * 2.0 ** -g == vmax
    rng = np.random.default_rng(9000 + seed)
    table = np.ldexp(rng.integers(-top, top + 1, TABLE_LEN).astype(np.float64), -g)
    table[used[0]], table[used[1]] = vmax, -vmax
    assert np.abs(table).max() == vmax
    return table


def constant_table(value):
    return np.full(TABLE_LEN, float(value))


def alternating_table(value=1024.0):
    """+value in the even bins, -value in the odd ones."""
    return np.tile(np.where(np.arange(20) % 2 == 0, float(value), -float(value)), TABLE_LEN // 20)


SIGN_TABLES = [("-1024", lambda: constant_table(-1024.0), -1024.0), ("+1024", lambda: constant_table(1024.0), 1024.0),
               ("alternating", alternating_table, None)]


def declined_table(kind, used, poses_idx):
    """The vmax = 10 ladder with ONE entry the block-major path cannot take -- the next f64 above 1024, an infinity, a NaN -- in a
    type pair and bin that some poses of the case read and others do not.  Returns (table, entry)."""
    reads = sum(np.isin(used, idx).astype(np.int64) for idx in poses_idx)
    entry = used[np.flatnonzero((reads > 0) & (reads < len(poses_idx)))[0]]
    table = ladder_table(10.0, 20, used, seed=3)
    table[entry] = {"above": np.nextafter(1024.0, np.inf), "inf": np.inf, "nan": np.nan}[kind]
    return table, int(entry)


def uniform_table(vmax=1000.0, seed=17):
    """NOT dyadic: uniform f64 values in (-vmax, vmax), as a real table's are to the fixed point."""
    return np.random.default_rng(seed).uniform(-vmax, vmax, TABLE_LEN)


GUARD_G = 20


def guard_table(used):
    return ladder_table(10.0, GUARD_G, used, seed=5)


def kept_poses(case, orc):
    """The knife-edge guards of reference (2): a pose stays if the restatement's pair count equals the oracle's stats[5] AND its
    integer sum on a dyadic table equals the oracle's stats[0] exactly.  Returns (mask, share left out); asserts the cap."""
    idx = case.idx(orc)
    table = guard_table(case.used(orc))
    ints = dyadic_ints(table, GUARD_G)
    cpu = case.cpu(orc, table)
    keep = np.zeros(len(case.poses), dtype=bool)
    for k, p in enumerate(case.poses):
        _, st = cpu.energy_ex_row(p)
        s = isum(ints[idx[k]])
        assert len(idx[k]) * int(np.abs(ints).max()) < 2 ** 53
        keep[k] = len(idx[k]) == int(st[5]) and np.ldexp(float(s), -GUARD_G) == st[0]
    share = 1.0 - keep.mean()
    print("TABLES %-32s left out by the knife-edge guards: %d of %d poses (%.1f %%)" % (case.label, (~keep).sum(), len(keep), 100.0 * share))
    assert keep.any() and share <= MAX_LEFT_OUT, (case.label, share)
    return keep, share


# ---- the device side ---------------------------------------------------------------------------------------------------

def evaluate(scorer, poses):
    """(energies of a plain launch, energies and in-cutoff pair counts of a counting launch)."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n = len(poses)
    d_poses = torch.from_numpy(np.ascontiguousarray(poses)).to(dev)
    d_out = torch.zeros(n, dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    scorer.energy_batch_device(n, d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), None, d_cnt.data_ptr())
    torch.cuda.synchronize()
    return scorer.energy_batch(poses), d_out.cpu().numpy(), d_cnt.cpu().numpy().astype(np.int64)


def oracle_rows(cpu, poses):
    rows = [cpu.energy_ex_row(p) for p in poses]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])


def hold_dyadic(pkg, orc, case, table, g, klass, label, routes=ROUTES, poses=None, known_raw=None):
    """A dyadic table on every route: the route's name, energies within the tail's roundings of the oracle's (both launches),
    pair counts equal.  known_raw(count) -> the raw sum that an identity of the table gives, checked against the DEVICE's counts."""
    poses = case.poses if poses is None else poses
    want, stats = oracle_rows(case.cpu(orc, table), poses)
    raw, counts = stats[:, 0], stats[:, 5].astype(np.int64)
    top = int(np.abs(dyadic_ints(table, g)).max())
    assert int(counts.max()) * top < 2 ** 53, "the dyadic premise: pairs * max|v| * 2^g < 2^53"
    for env, name in routes:
        hip = case.hip(pkg, table, env)
        assert hip.kernel_info()["pair_kernel_name"] == name, (label, env)
        plain, counted, cnt = evaluate(hip, poses)
        assert np.array_equal(cnt, counts), (label, env)
        hold_exact("%s %s %s" % (case.label, label, name), klass, plain, want, raw)
        hold_exact("%s %s %s (counting launch)" % (case.label, label, name), klass, counted, want, raw)
        if known_raw is not None:   # independent of the oracle's sum: the table's identity on the device's own counts
            mine = np.array([tail(known_raw(int(c)), st) for c, st in zip(cnt, stats)])
            hold_exact("%s %s %s (identity)" % (case.label, label, name), klass, plain, mine, np.array([known_raw(int(c)) for c in cnt], dtype=np.float64))
    return want, stats


# ---- 1. the magnitude ladder -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("rung", LADDER, ids=LADDER_IDS)
@pytest.mark.parametrize("name", ["1ppe", "1k4c"])
def test_magnitude_ladder(pkg, orc, name, rung, route):
    """e = 0 (the max(vmax, 1) clamp, and a table far below 1), vmax == 2^e exactly and just above it, e = 10 at kBmFixLimit:
    all stay on the block-major path by default, and all three routes give the oracle's energy to the tail's roundings.
    (vmax = 2^-30: the sum is ~1e-5 next to 4.7, so the energy shows it through some 6 digits only -- an error of a whole table
    value per pair would still pass any relative tolerance; the ulp bound is what makes this rung worth running.)"""
    vmax, g, e = rung
    pkg.init(0)
    case = fixture_case(name, orc)
    table = ladder_table(vmax, g, case.used(orc))
    assert g <= 44 - e
    hold_dyadic(pkg, orc, case, table, g, "ladder", "vmax %s" % LADDER_IDS[LADDER.index(rung)], routes=[route])


@pytest.mark.parametrize("kind", ["above", "inf", "nan"])
@pytest.mark.parametrize("name", ["1ppe", "1k4c", "2uuy"])
def test_tables_the_fixed_point_cannot_take_run_the_packed_kernel(pkg, orc, name, kind):
    """One entry at nextafter(1024), +inf or NaN: `bm_accepts` declines, rigid or flexing, and the pose-major kernel carries
    the value as the reference does (src/dfire.rs:338).  Its sums are f64 in another order: `rel_err` against the oracle, as for
    that kernel everywhere.  A pose that reads an inf / NaN entry is non-finite on both sides; the others are compared."""
    pkg.init(0)
    case = fixture_case(name, orc)
    table, entry = declined_table(kind, case.used(orc), case.idx(orc))
    reads = np.array([bool(np.any(i == entry)) for i in case.idx(orc)])
    assert reads.any() and not reads.all()
    want, stats = oracle_rows(case.cpu(orc, table), case.poses)
    hip = case.hip(pkg, table)
    assert hip.kernel_info()["pair_kernel_name"] == PACKED
    plain, counted, cnt = evaluate(hip, case.poses)
    assert np.array_equal(cnt, stats[:, 5].astype(np.int64))
    for got in (plain, counted):
        if kind == "above":
            assert rel_err(got, want) < REL_TOL
        else:
            assert np.array_equal(np.isfinite(want), ~reads)
            assert np.array_equal(np.isfinite(got), ~reads)
            assert rel_err(got[~reads], want[~reads]) < REL_TOL


# ---- 2. sign extremes at e = 10 --------------------------------------------------------------------------------------

def _sign_extremes(pkg, orc, case, routes):
    for label, make, value in SIGN_TABLES:
        known = None if value is None else (lambda count, v=value: v * count)
        _, stats = hold_dyadic(pkg, orc, case, make(), 0, "sign", label, routes=routes, known_raw=known)
        if value is not None:
            assert np.array_equal(stats[:, 0], value * stats[:, 5])
    return stats


@pytest.mark.parametrize("name", ["1ppe", "1k4c", "2uuy"])
def test_sign_extremes_on_the_fixtures(pkg, orc, name):
    """Every value -1024, every value +1024, the sign alternating with the bin: at e = 10 a table value is +-2^44 fixed-point
    units and a block's 32-pair half-sum reaches +-2^49 -- the largest borrow out of (or carry towards) the marker field that
    `finish_batch` has to undo.  raw == +-1024 * count, also on the counting launch's own counts."""
    pkg.init(0)
    _sign_extremes(pkg, orc, fixture_case(name, orc), ROUTES)


@pytest.mark.parametrize("restraints", [False, True], ids=["free", "restrained"])
@pytest.mark.parametrize("n_rec,n_lig", [(65, 63), (200, 130), (1100, 300)])
def test_sign_extremes_on_overlapping_random_molecules(pkg, orc, tmp_path, n_rec, n_lig, restraints):
    """... where whole 8 x 8 blocks lie inside the cutoff (the four overlapping poses of test_random_molecules_match_oracle);
    with restraints the tracked blocks carry markers in bins 0 and 1 on top."""
    pkg.init(0)
    case = random_rigid_case(tmp_path, n_rec, n_lig, restraints)
    stats = _sign_extremes(pkg, orc, case, ROUTES)
    assert stats[:4, 5].min() > n_rec * n_lig / 3, "the overlapping poses should hold a third of all pairs"


@pytest.mark.parametrize("restraints", [False, True], ids=["free", "restrained"])
@pytest.mark.parametrize("n_rec,n_lig,k_rec,k_lig", [(65, 63, 0, 10), (200, 130, 10, 10), (513, 65, 7, 1)])
def test_sign_extremes_on_flexing_random_molecules(pkg, orc, tmp_path, n_rec, n_lig, k_rec, k_lig, restraints):
    """The ANM form of the block-major path, a tenth of the poses wild."""
    pkg.init(0)
    _sign_extremes(pkg, orc, random_anm_case(tmp_path, n_rec, n_lig, k_rec, k_lig, restraints), ROUTES)


# ---- 3. arbitrary tables against the path's own specification --------------------------------------------------------

def fixed_point_reference(case, orc, table, scale):
    """(energies, raw sums, extra allowance) the block-major path is SPECIFIED to give: sum of llrint(v * scale) over the
    restated pairs / scale, then the tail with the oracle's fractions."""
    fixed = np.rint(table * scale).astype(np.int64)           # (v * 2^k is exact; rint = llrint's round-half-even)
    _, stats = oracle_rows(case.cpu(orc, table), case.poses)
    want, raws, extra = [], [], []
    poses_idx = case.idx(orc)
    tiles = (case.n_lig + 63) // 64
    for idx, st in zip(poses_idx, stats):
        s = isum(fixed[idx])
        raw = float(s) / scale                                # (float(s): correctly rounded; / 2^k: exact)
        # beyond 53 significant bits the gather's f64 adds round: one spacing of the raw term per ligand tile, plus one
        extra.append(0.0 if fits_53_bits(s) else (tiles + 1) * np.spacing(abs(raw) * 0.0157))
        raws.append(raw)
        want.append(tail(raw, st))
    return np.array(want), np.array(raws), np.array(extra), stats


@pytest.mark.parametrize("which", ["synthetic", "uniform1000"])
@pytest.mark.parametrize("name", ["1ppe", "1k4c", "2uuy"])
def test_block_major_sums_equal_their_fixed_point_specification(pkg, orc, table, name, which):
    """The stock synthetic table (e = 4) and a non-dyadic one at |v| <= 1000 (e = 10): the GPU energy against integer
    arithmetic in Python, and -- DESIGN section 3's claim -- bit-identical however the launch is cut up (passes of 16 poses,
    jobs of 64 entries)."""
    pkg.init(0)
    case = fixture_case(name, orc)
    keep, _ = kept_poses(case, orc)
    t = table if which == "synthetic" else uniform_table()
    s = case.cpu(orc, t)
    count, extra_bits, scale = pkg.dfire_bm_fix_scale(s.model(0)["coordinates"], 15.0 + 60.0, float(np.abs(t).max()))
    assert extra_bits == 0 and scale == (2.0 ** 40 if which == "synthetic" else 2.0 ** 34)
    want, raws, extra, stats = fixed_point_reference(case, orc, t, scale)
    hip = case.hip(pkg, t)
    assert hip.kernel_info()["pair_kernel_name"] == BM
    plain, counted, cnt = evaluate(hip, case.poses)
    assert np.array_equal(cnt, stats[:, 5].astype(np.int64))
    assert np.array_equal(plain, counted)
    hold_exact("%s %s" % (name, which), "reference", plain[keep], want[keep], raws[keep], extra[keep])
    for env in ({"LIGHTDOCK_BM_CHUNK": "16"}, {"LIGHTDOCK_BM_PART_CAP": "64"}):
        other = case.hip(pkg, t, env)
        assert other.kernel_info()["pair_kernel_name"] == BM
        assert np.array_equal(other.energy_batch(case.poses), plain), env


# ---- 4. x > 0 and the 63-bit bound -------------------------------------------------------------------------------------

BALL_SIZES = [500, 2000, 8191, 8192, 16382, 16383]      # (in this order: the small ones first)
BALL_EXTRA_BITS = {500: 0, 2000: 0, 8191: 0, 8192: 1, 16382: 1, 16383: 2}


def _ball(pkg, orc, case, n_rec, n_lig, routes):
    pairs = n_rec * n_lig
    for label, make, value in SIGN_TABLES[:2]:
        _, stats = hold_dyadic(pkg, orc, case, make(), 0, "ball", label, routes=routes, known_raw=lambda count, v=value: v * count)
        assert np.all(stats[:, 5] == pairs), "every pair of the ball is inside the cutoff"
        assert np.all(stats[:, 0] == value * pairs)
    hold_dyadic(pkg, orc, case, ladder_table(10.0, 20, case.used(orc)), 20, "ball", "vmax 10", routes=routes)


@pytest.mark.parametrize("n_lig", [64, 130])
@pytest.mark.parametrize("n_rec", BALL_SIZES)
def test_crowded_receptor_takes_bits_off_the_scale(pkg, orc, tmp_path, n_rec, n_lig):
    """More than 8191 receptor atoms within reach of one ligand tile: x = 1, 2 bits come off the scale, and the sums stay exact
    (g = 20 <= 44 - e - x).  At 8191 atoms and +-1024 a (row, ligand tile) sum is +-8191 * 2^50, directly under the 2^63 the
    guard exists for; with 130 ligand atoms the pose's total, 8191 * 130 * 2^44, passes 2^63 and has to survive the gather's
    f64 adds (exactly: few significant bits).  The other routes up to 2000 atoms."""
    pkg.init(0)
    case = ball_case(tmp_path, n_rec, n_lig)
    _ball(pkg, orc, case, n_rec, n_lig, ROUTES if n_rec <= 2000 else ROUTES[:1])
    if n_rec == 8191:
        assert 64 * n_rec * 2 ** 44 < 2 ** 63 <= 64 * (n_rec + 1) * 2 ** 44
    if n_rec == 8191 and n_lig == 130:
        assert n_rec * n_lig * 2 ** 44 > 2 ** 63


def test_crowded_receptor_with_restraints(pkg, orc, tmp_path):
    """The ball at 2000 atoms with active restraints on both sides: blocks of tracked atoms send their pairs of bins 0 and 1
    to the exact path too."""
    pkg.init(0)
    case = ball_case(tmp_path, 2000, 130, restraints=True)
    _ball(pkg, orc, case, 2000, 130, ROUTES)
