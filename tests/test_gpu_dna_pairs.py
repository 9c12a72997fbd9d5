"""pose_energy_pairs<1, *> (DNA and PYDOCK; csrc/kernels/pose_energy.hip) held to a derived error bound on synthetic shapes.

Everything goes through Scorer.from_arrays.  The reference is tests/dna_reference.py: f64 terms by the reference's
formulas on the kernel's own d2, summed exactly, with a per-pose bound built from the reference's terms alone (reciprocal
by v_rcp_f64 and one Newton step, order of the sum, tail).  tests/test_dna_reference_cpu.py holds that restatement to the
oracle and checks, without a GPU, that the inputs used here reach every clamp and cutoff and that the bound is far below
one pair at the cutoff.

What each shape reaches (receptor chunk 256 unless LIGHTDOCK_CHUNK_ATOMS says otherwise; split_j when the ligand's 64-atom
groups are fewer than 16 and no multiple of 4):
  1 x 1            one pair, split_j with 3 empty waves
  3 x 65           split_j, quarter = 1, last group of 1 atom
  64 x 64          one full group
  255 x 256        4 groups, not split; 1 chunk
  256 x 257        5 groups, split; 1 chunk exactly full
  257 x 63         2 ragged chunks
  513 x 960        3 chunks; 15 groups, split
  448 x 64   @64   7 partials (fewer than the finish lanes)
  512 x 65   @64   8 partials
  513 x 130  @64   9 partials, chunk_atoms = 57
  1025 x 1025 @64  17 partials; 17 groups, not split, tail group of 1 atom"""
import numpy as np
import pytest

import dna_reference as dr

pytestmark = pytest.mark.gpu

DNA_KEYS = ("coordinates", "ele_charges", "vdw_charges", "vdw_radii", "membrane", "restraint_offsets", "restraint_atoms", "nmodes", "num_anm")
SENTINEL = -12345.0


def build(pkg, monkeypatch, shape, rec, lig, method="dna", use_anm=False):
    """The scorer of one shape; the chunk setting is read when the scorer is built.  Asserts the kernel and its chunks."""
    pkg.init(0)
    if shape[2] is None:
        monkeypatch.delenv("LIGHTDOCK_CHUNK_ATOMS", raising=False)
    else:
        monkeypatch.setenv("LIGHTDOCK_CHUNK_ATOMS", str(shape[2]))
    pick = lambda m: {k: m[k] for k in DNA_KEYS if k in m}
    hip = pkg.Scorer.from_arrays(method, pick(rec), pick(lig), use_anm=use_anm)
    info = hip.kernel_info()
    assert info["pair_kernel_name"].startswith("pose_energy_pairs<1") and info["receptor_chunks"] == shape[3], (shape, info)
    assert hip.num_atoms(0) == shape[0] and hip.num_atoms(1) == shape[1]
    return hip


def check_within_bound(got, want, where):
    """|got - want| <= bound for every pose whose reference is finite, NaN where it is NaN; no pose is left out.  Returns
    the largest |got - want| / bound."""
    assert len(got) == len(want)
    worst = 0.0
    for p, w in enumerate(want):
        if w["nan"]:
            assert np.isnan(got[p]), (where, p, got[p])
            continue
        err = abs(got[p] - w["energy"])
        assert not np.isnan(got[p]) and err <= w["bound"], (where, p, got[p], w["energy"], err, w["bound"])
        if w["bound"] > 0.0:
            worst = max(worst, err / w["bound"])
    return worst


def device_run(torch, hip, poses, active=None, counts=False):
    """energy_batch_device on torch's current stream -> (energies over a sentinel, pair counts or None)."""
    dev = torch.device("cuda:0")
    n = len(poses)
    d_poses = torch.from_numpy(np.ascontiguousarray(poses)).to(dev)
    d_out = torch.full((n,), SENTINEL, dtype=torch.float64, device=dev)
    d_active = None if active is None else torch.from_numpy(active).to(dev)
    d_cnt = torch.full((n,), -1, dtype=torch.int32, device=dev) if counts else None
    hip.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        hip.energy_batch_device(n, d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), None if d_active is None else d_active.data_ptr(),
                                None if d_cnt is None else d_cnt.data_ptr())
        torch.cuda.synchronize()
    finally:
        hip.set_stream(0)
    return d_out.cpu().numpy(), None if d_cnt is None else d_cnt.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("shape", dr.SHAPES, ids=dr.shape_id)
def test_energies_within_the_derived_bound(pkg, orc, monkeypatch, shape):
    """Largest |got - want| / bound seen on the MI355X: 1x1 3.2e-2, 3x65 7.5e-3, 64x64 2.1e-3, 255x256 1.7e-4, 256x257 1.8e-4,
    257x63 9.2e-4, 513x960 1.1e-5, 448x64@64 3.4e-4, 512x65@64 1.7e-4, 513x130@64 1.1e-4, 1025x1025@64 5.4e-6."""
    rec, lig, poses, want = dr.shape_reference(orc, shape)
    hip = build(pkg, monkeypatch, shape, rec, lig)
    assert hip.pose_len == 7
    got = hip.energy_batch(poses)
    worst = check_within_bound(got, want, dr.shape_id(shape))
    print("%s: largest |got - want| / bound = %.2e over %d poses" % (dr.shape_id(shape), worst, len(poses)))
    assert got[dr.ROW_FAR] == 0.0 and want[dr.ROW_FAR]["pairs"] == 0        # nothing within 30 A: zero, not almost zero
    if shape[:2] == (1, 1):
        torch = pytest.importorskip("torch")
        at_900, at_100, out_900, out_100 = (want[r] for r in (dr.ROW_900, dr.ROW_100, dr.ROW_OUTSIDE_900, dr.ROW_OUTSIDE_100))
        # d2 == 900 counts: the electrostatic term alone, and it is there
        assert at_900["vdw"] == 0.0 and got[dr.ROW_900] != 0.0 and abs(got[dr.ROW_900]) > 1000.0 * at_900["bound"]
        # d2 == 100 counts for van der Waals: the term is many bounds large, so an energy within the bound has it
        assert abs(at_100["vdw"]) > 1000.0 * at_100["bound"] and got[dr.ROW_100] != -(at_100["elec"] * 332.0 / 4.0)
        # 2^-40 outside 900: nothing at all; 2^-40 outside 100: the electrostatic term and no van der Waals term, which
        # would be as large as the one at 100
        assert got[dr.ROW_OUTSIDE_900] == 0.0 and out_900["pairs"] == 0
        assert out_100["vdw"] == 0.0 and abs(got[dr.ROW_OUTSIDE_100] + out_100["elec"] * 332.0 / 4.0) <= out_100["bound"]
        assert abs(at_100["vdw"]) > 1000.0 * out_100["bound"]
        _, cnt = device_run(torch, hip, poses, counts=True)
        assert [int(cnt[r]) for r in (dr.ROW_900, dr.ROW_100, dr.ROW_IFACE, dr.ROW_OUTSIDE_900)] == [1, 1, 1, 0]


@pytest.mark.parametrize("shape", [dr.SHAPES[1], dr.SHAPES[4], dr.SHAPES[9]], ids=dr.shape_id)
def test_pair_counts_active_mask_and_both_instantiations(pkg, orc, monkeypatch, shape):
    assert [s[:3] for s in (dr.SHAPES[1], dr.SHAPES[4], dr.SHAPES[9])] == [(3, 65, None), (256, 257, None), (513, 130, 64)]
    torch = pytest.importorskip("torch")
    rec, lig, poses, want = dr.shape_reference(orc, shape)
    hip = build(pkg, monkeypatch, shape, rec, lig)
    plain, none = device_run(torch, hip, poses)
    counted, cnt = device_run(torch, hip, poses, counts=True)
    assert none is None and np.array_equal(plain, counted, equal_nan=True)          # COUNT changes no bit
    assert np.array_equal(plain, hip.energy_batch(poses), equal_nan=True)
    check_within_bound(plain, want, dr.shape_id(shape))
    assert np.array_equal(cnt, np.array([w["pairs"] for w in want], dtype=np.int64))
    active = np.ones(len(poses), dtype=np.uint8)
    active[::3] = 0
    on = active == 1
    for counts in (False, True):
        masked, mcnt = device_run(torch, hip, poses, active=active, counts=counts)
        assert np.all(masked[~on] == SENTINEL) and np.array_equal(masked[on], plain[on], equal_nan=True)
        if counts:
            assert np.array_equal(mcnt[on], cnt[on]) and np.all(mcnt[~on] == -1)
    assert on[dr.ROW_COINCIDENT] and np.isnan(plain[dr.ROW_COINCIDENT])                # the NaN pose is among the live ones


@pytest.mark.parametrize("shape", [dr.SHAPES[1], dr.SHAPES[5]], ids=dr.shape_id)
def test_energy_does_not_depend_on_the_batch(pkg, orc, monkeypatch, shape):
    rec, lig, poses, want = dr.shape_reference(orc, shape)
    hip = build(pkg, monkeypatch, shape, rec, lig)
    whole = hip.energy_batch(poses)
    check_within_bound(whole, want, dr.shape_id(shape))
    assert np.array_equal(hip.energy_batch(poses[::-1])[::-1], whole, equal_nan=True)
    for p, row in enumerate(poses):
        assert np.array_equal(hip.energy_batch(row[None]), whole[p:p + 1], equal_nan=True), p
        assert np.array_equal([hip.energy(row[:3], row[3:7])], whole[p:p + 1], equal_nan=True), p


def test_tail_restraints_and_membrane(pkg, orc, monkeypatch):
    rec, lig, poses, want = dr.tail_case(orc)
    live = [w for w in want if not w["nan"]]
    assert {w["rec_restraints"] for w in live} == {0.0, 0.5, 1.0} and {w["lig_restraints"] for w in live} == {0.0, 1.0}
    assert any(w["membrane"] > 0.0 for w in live)
    assert int(lig["restraint_atoms"][-1]) == dr.TAIL_SHAPE[1] - 1 and dr.TAIL_SHAPE[1] % 64 == 2      # in the padded tail group
    hip = build(pkg, monkeypatch, dr.TAIL_SHAPE, rec, lig)
    got = hip.energy_batch(poses)
    worst = check_within_bound(got, want, "tail")
    print("tail 257x130: largest |got - want| / bound = %.2e; penalties %s" % (worst, sorted({w["membrane"] for w in live})))
    # the penalty and the fractions are many bounds large: an energy within the bound has the right ones
    for w in live:
        if w["membrane"] > 0.0:
            assert 999.0 * 0.2 > 1e6 * w["bound"]
        if w["rec_restraints"] + w["lig_restraints"] > 0.0:
            assert 0.5 * abs(w["score"]) > 1e6 * w["bound"]


@pytest.mark.parametrize("modes", dr.ANM_MODES, ids=lambda m: "%d+%d" % m)
@pytest.mark.parametrize("shape", dr.ANM_SHAPES, ids=dr.shape_id)
def test_anm_on_one_side_or_both(pkg, orc, monkeypatch, shape, modes):
    rec, lig, poses, want = dr.anm_case(orc, shape, *modes)
    hip = build(pkg, monkeypatch, shape, rec, lig, use_anm=True)
    assert hip.pose_len == 7 + sum(modes) == poses.shape[1] and not np.isnan(poses).any()
    got = hip.energy_batch(poses)
    worst = check_within_bound(got, want, (shape, modes))
    print("anm %s %s: largest |got - want| / bound = %.2e" % (dr.shape_id(shape), modes, worst))
    # the modes matter: the rigid molecules at the same rows score differently
    rigid = build(pkg, monkeypatch, shape, {k: v for k, v in rec.items() if k not in ("nmodes", "num_anm")},
                  {k: v for k, v in lig.items() if k not in ("nmodes", "num_anm")}).energy_batch(poses)
    assert not np.array_equal(rigid, got, equal_nan=True)


def test_pydock_is_the_same_kernel(pkg, orc, monkeypatch):
    shape = dr.SHAPES[2]
    assert shape[:2] == (64, 64)
    rec, lig, poses, want = dr.shape_reference(orc, shape)
    dna = build(pkg, monkeypatch, shape, rec, lig).energy_batch(poses)
    pydock = build(pkg, monkeypatch, shape, rec, lig, method="pydock").energy_batch(poses)
    assert np.array_equal(dna, pydock, equal_nan=True)
    check_within_bound(pydock, want, "pydock")
