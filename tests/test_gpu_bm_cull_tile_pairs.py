"""dfire_bm_cull's step loop over the receptor tiles that survive the 64 x 64 box test, at the shapes at which a
change of that walk can go wrong, against the oracle.  The loop was measured in several forms -- the surviving tiles two a trip, as
a lane-distributed list, the hits recorded without a branch or by exec-masked moves (tools/experiments/r15_cull_step_variants.patch)
-- and every form has to pass this file; the form kept walks one tile a step and reads a subtile's box as two 16-byte pieces.

What can go wrong: an odd number of survivors (a walk that takes two tiles a trip pairs the last one with itself and must drop the
second ballot: a hit recorded twice doubles that tile pair's sums and pair counts, a dropped one loses them); a second ballot
(`base` = 64) that holds exactly one or exactly two tiles; a ballot with no survivor; a test held against another box's reach
instead of its own (a receptor subtile whose rows of the potential are zero reaches 2.45 A or nothing, its neighbour 15 A: the
reach travels in the second 16-byte piece of the box).

Shapes.  Receptors of 1, 2, 3, 63, 64, 65 and 66 tiles (64 atoms a tile, the last one ragged) in a cube of 24 A, ligands of one
full tile and of one tile plus one atom in a cube of 18 A, as test_gpu_parity.py's random molecules.  Pose 0 is far away (no
survivor, energy 4.7); poses 1-8 overlap the receptor: the full ligand tile's box then spans the ligand's cube, within 15 A of
every receptor tile's box, so ALL n_rt tiles survive -- an odd and an even count by the receptor's size, 64 + 1 and 64 + 2 over two
ballots -- while the one-atom tile and the poses further out (translations up to 22 A an axis) reach only some of them.  Batches
of 1, 9 and 65 poses: a partial item, and, as every launch here is small, two poses an item.

That claim is checked, not assumed: the library's atom order (`dfire_tile_layout`, as tests/test_host_cpu.py rebuilds the subtiles
from it) and the oracle's model coordinates give every pose's tiles and subtiles on the CPU in f64; the exact boxes of a full ligand
tile must come within 15 A of ALL n_rt receptor tile boxes in each of poses 1-8 (the kernel's boxes are those, widened), and the
replay's in-cutoff pairs must be the oracle's.

Tolerance: test_gpu_parity.py's for the block-major path (bm_err < REL_TOL).  In-cutoff pair counts are equalities: the counting
launch lists every block within the full cutoff, so a tile pair lost or listed twice shows in them.  `last_block_counts` of a pose
is at least the number of (ligand subtile, receptor subtile) blocks that hold a pair within 15 A -- counted by the same replay --
and at most every block of the tile grid."""
import numpy as np
import pytest

from test_gpu_parity import REL_TOL, _counts_of, _random_molecule, _write_pdb, bm_err

pytestmark = pytest.mark.gpu

BM = "dfire_bm_pairs"
N_POSES = 65
FAR = 0
BATCHES = (slice(0, 1), slice(1, 2), slice(0, 9), slice(0, N_POSES))   # 1 pose (far; near), 9, 65


def _poses(rng):
    poses = np.zeros((N_POSES, 7))
    poses[:, :3] = rng.uniform(-22, 22, (N_POSES, 3))
    poses[1:9, :3] = rng.uniform(-2, 2, (8, 3))
    q = rng.normal(size=(N_POSES, 4))
    poses[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    poses[FAR, :3] = (500.0, -300.0, 200.0)
    return poses


def _ordered(pkg, model, far):
    """A molecule's atoms in the scorer's slots (64 a tile, 8 a subtile; padding slots far away), and which slots hold an atom."""
    order, _ = pkg.dfire_tile_layout(model["coordinates"], model["dfire_types"])
    pad = order == 0xFFFFFFFF
    xyz = model["coordinates"][np.where(pad, 0, order).astype(np.int64)].copy()
    xyz[pad] = far
    return xyz, ~pad


def _boxes(xyz, valid, size):
    c, v = xyz.reshape(-1, size, 3), valid.reshape(-1, size)
    return np.where(v[..., None], c, np.inf).min(1), np.where(v[..., None], c, -np.inf).max(1)


def _replay(pkg, cpu, poses):
    """Per pose, on the CPU in f64: pairs within 15 A, 8 x 8 blocks that hold one, and the most receptor tiles whose box comes
    within 15 A of the box of one ligand tile."""
    rc, rv = _ordered(pkg, cpu.model(0), 1e9)
    lc, lv = _ordered(pkg, cpu.model(1), -1e9)
    r_lo, r_hi = _boxes(rc, rv, 64)
    pairs, blocks, survivors = [], [], []
    for p in poses:
        w, x, y, z = p[3:7] / np.linalg.norm(p[3:7])
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        l = lc @ R.T + p[:3]
        d2 = ((l[:, None, :] - rc[None, :, :]) ** 2).sum(-1)
        within = (d2 <= 225.0) & lv[:, None] & rv[None, :]
        pairs.append(within.sum())
        blocks.append(within.reshape(len(l) // 8, 8, len(rc) // 8, 8).any(axis=(1, 3)).sum())
        l_lo, l_hi = _boxes(l, lv, 64)
        gap = np.maximum(0, np.maximum(l_lo[:, None] - r_hi[None], r_lo[None] - l_hi[:, None]))
        survivors.append(((gap ** 2).sum(-1) <= 225.0).sum(1).max())
    return np.array(pairs, dtype=np.int64), np.array(blocks, dtype=np.int64), np.array(survivors, dtype=np.int64)


class Complex:
    """A random rigid complex, its poses and the oracle's answers, made once and left unchanged."""

    def __init__(self, pkg, orc, table, directory, n_rec, n_lig, seed):
        rng = np.random.default_rng(seed)
        rec, lig = str(directory / "rec.pdb"), str(directory / "lig.pdb")
        rec_atoms = _random_molecule(rng, n_rec, 24.0, "A")
        lig_atoms = _random_molecule(rng, n_lig, 18.0, "B")
        _write_pdb(rec, rec_atoms)
        _write_pdb(lig, lig_atoms)
        kw = dict(rec_active=["A.%s.%d" % (rec_atoms[0][1], rec_atoms[0][3])],
                  lig_active=["B.%s.%d" % (lig_atoms[-1][1], lig_atoms[-1][3])], potential=table)
        self.n_rec, self.n_lig = n_rec, n_lig
        self.poses = _poses(rng)
        self.cpu = orc.Scorer("dfire", rec, lig, **kw)
        self.hip = pkg.Scorer.from_pdb("dfire", rec, lig, **kw)
        ex = [self.cpu.energy_ex_row(p) for p in self.poses]
        self.want = np.array([e for e, _ in ex], dtype=np.float64)
        self.pairs = np.array([s[5] for _, s in ex]).astype(np.int64)
        self.n_rt = -(-n_rec // 64)
        self.replay_pairs, self.blocks_with_a_pair, self.survivors = _replay(pkg, self.cpu, self.poses)
        for a in (self.poses, self.want, self.pairs, self.replay_pairs, self.blocks_with_a_pair, self.survivors):
            a.setflags(write=False)


def _check(torch, c):
    assert c.hip.kernel_info()["pair_kernel_name"] == BM
    assert c.hip.num_atoms(0) == c.n_rec and c.hip.num_atoms(1) == c.n_lig
    assert c.pairs[FAR] == 0 and c.want[FAR] == 4.7
    assert (c.pairs[1:9] > 0).all()
    assert np.array_equal(c.replay_pairs, c.pairs)                  # the replay poses and counts as the oracle does
    assert np.all(c.survivors[1:9] == c.n_rt), c.survivors[1:9]     # poses 1-8: every receptor tile survives a ligand tile's test
    assert c.survivors[FAR] == 0 and c.blocks_with_a_pair[FAR] == 0
    assert len(np.unique(c.survivors)) > 2 or c.n_rt < 63, "the poses further out reach only some of the tiles"
    all_blocks = (-(-c.n_rec // 64) * 8) * (-(-c.n_lig // 64) * 8)
    for rows in BATCHES:
        poses, want, pairs, with_a_pair = c.poses[rows], c.want[rows], c.pairs[rows], c.blocks_with_a_pair[rows]
        got = c.hip.energy_batch(poses)
        err = bm_err(got, want)
        counted, counts = _counts_of(torch, c.hip, poses)
        blocks = c.hip.last_block_counts(len(poses)).astype(np.int64)
        print("%d x %d atoms, %d poses: err %.2e, counting launch %.2e, pairs %d..%d, blocks %d..%d of %d, blocks - those with a pair %d..%d"
              % (c.n_rec, c.n_lig, len(poses), err, bm_err(counted, want), pairs.min(), pairs.max(), blocks.min(), blocks.max(), all_blocks,
                 (blocks - with_a_pair).min(), (blocks - with_a_pair).max()))
        assert err < REL_TOL
        assert bm_err(counted, want) < REL_TOL
        assert np.array_equal(counts.astype(np.int64), pairs)
        assert np.all(blocks >= with_a_pair) and np.all(blocks <= all_blocks)
        if rows.start == FAR:
            assert got[0] == 4.7 and blocks[0] == 0


@pytest.mark.parametrize("n_lig", [64, 65])
@pytest.mark.parametrize("rec_tiles", [1, 2, 3, 63, 64, 65, 66])
def test_tile_pairs_over_receptor_sizes(pkg, orc, table, tmp_path, rec_tiles, n_lig):
    torch = pytest.importorskip("torch")
    pkg.init(0)
    n_rec = rec_tiles * 64 - 13          # (a ragged last tile: 51 atoms, its last subtile 3)
    _check(torch, Complex(pkg, orc, table, tmp_path, n_rec, n_lig, 7000 + 10 * rec_tiles + n_lig))


def test_tile_pairs_with_quiet_receptor_subtiles(pkg, orc, table, tmp_path):
    """The rows of most receptor types zeroed: a subtile of such atoms only is listed within the interface distance (the ligand has
    a restraint), its neighbours within the cutoff -- neighbouring boxes of a tile are held against different reaches.  65 receptor
    tiles: an odd count over two ballots."""
    torch = pytest.importorskip("torch")
    pkg.init(0)
    n_rec, n_lig = 65 * 64 - 13, 65
    probe = Complex(pkg, orc, table, tmp_path, n_rec, n_lig, 7777)
    rng = np.random.default_rng(7778)
    rec_types = np.unique(probe.cpu.model(0)["dfire_types"])
    silent = rng.permutation(rec_types)[: int(0.93 * len(rec_types))]
    t = table.copy()
    t.reshape(169, 169, 20)[silent, :, :] = 0.0
    c = Complex(pkg, orc, t, tmp_path, n_rec, n_lig, 7777)
    quiet = c.hip.bm_quiet_subtiles()
    assert 8 <= quiet <= 65 * 8 - 8, quiet          # both kinds of subtile, many of each
    assert probe.hip.bm_quiet_subtiles() == 0
    assert np.array_equal(c.pairs, probe.pairs)     # (the cutoff does not look at the table)
    _check(torch, c)
