"""The premises of tests/test_gpu_dfire_tables.py, proved without a GPU: on the very poses and tables the GPU tests use, the
oracle's raw DFIRE sum (stats[0]) IS the integer sum of an independent numpy restatement -- so "exact reference" there is a
fact and not a hope --, the knife-edge guards leave out no more poses than their cap, and the host arithmetic that picks the
block-major path's fixed-point scale gives the exponent e and the extra bits x that each table class is built to reach."""
import numpy as np
import pytest

import test_gpu_dfire_tables as T


def _check_dyadic(case, orc, table, g, keep=None):
    """oracle stats[0] == integer restatement * 2^-g, stats[5] == its pair count, energy == the host tail of it: bit for bit."""
    ints = T.dyadic_ints(table, g)
    cpu = case.cpu(orc, table)
    for k, (p, idx) in enumerate(zip(case.poses, case.idx(orc))):
        if keep is not None and not keep[k]:
            continue
        e, st = cpu.energy_ex_row(p)
        assert len(idx) * int(np.abs(ints).max()) < 2 ** 53          # the premise of "exact in any order"
        assert int(st[5]) == len(idx), (case.label, k)
        raw = np.ldexp(float(T.isum(ints[idx])), -g)
        assert st[0] == raw, (case.label, k, st[0], raw)
        assert e == T.tail(raw, st), (case.label, k)


@pytest.mark.parametrize("name", ["1ppe", "1k4c", "2uuy"])
def test_oracle_sums_are_the_integer_sums_on_the_fixtures(orc, name):
    """Ladder, sign and guard tables on the fixtures' poses; the left-out share printed and within its cap."""
    case = T.fixture_case(name, orc)
    keep, share = T.kept_poses(case, orc)
    assert share <= T.MAX_LEFT_OUT
    used = case.used(orc)
    for vmax, g, e in T.LADDER:
        table = T.ladder_table(vmax, g, used)
        assert g <= 44 - e
        assert np.isin(used[:2], case.idx(orc)[0]).all() and table[used[0]] == vmax and table[used[1]] == -vmax   # both signs at +-vmax, in rows the complex reads
        _check_dyadic(case, orc, table, g, keep)
    for label, make, value in T.SIGN_TABLES:
        _check_dyadic(case, orc, make(), 0, keep)
    _check_dyadic(case, orc, T.guard_table(used), T.GUARD_G, keep)


@pytest.mark.parametrize("kind", ["above", "inf", "nan"])
@pytest.mark.parametrize("name", ["1ppe", "1k4c", "2uuy"])
def test_declined_tables_split_the_poses_as_the_restatement_says(orc, name, kind):
    """The one entry beyond the fixed point sits in a type pair and bin that some poses read and others do not, and the oracle
    is non-finite exactly on the poses that the restatement says read an inf / NaN."""
    case = T.fixture_case(name, orc)
    table, entry = T.declined_table(kind, case.used(orc), case.idx(orc))
    reads = np.array([bool(np.any(i == entry)) for i in case.idx(orc)])
    assert reads.any() and not reads.all()
    want = case.cpu(orc, table).energy_rows(case.poses)
    assert np.array_equal(np.isfinite(want), np.ones(len(want), dtype=bool) if kind == "above" else ~reads)
    assert not (np.abs(table) <= 1024.0).all()


def _check_constant_tables(case, orc, all_pairs=None):
    for label, make, value in T.SIGN_TABLES:
        table = make()
        _check_dyadic(case, orc, table, 0)
        if value is not None:
            _, stats = T.oracle_rows(case.cpu(orc, table), case.poses)
            assert np.array_equal(stats[:, 0], value * stats[:, 5])
            if all_pairs is not None:
                assert np.all(stats[:, 5] == all_pairs)
    return stats


@pytest.mark.parametrize("restraints", [False, True], ids=["free", "restrained"])
@pytest.mark.parametrize("n_rec,n_lig", [(65, 63), (200, 130), (1100, 300)])
def test_oracle_sums_on_the_overlapping_random_molecules(orc, tmp_path, n_rec, n_lig, restraints):
    case = T.random_rigid_case(tmp_path, n_rec, n_lig, restraints)
    stats = _check_constant_tables(case, orc)
    print("TABLES %s: in-cutoff share of the overlapping poses %s" % (case.label, np.round(stats[:4, 5] / (n_rec * n_lig), 3)))
    assert stats[:4, 5].min() > n_rec * n_lig / 3     # (an input premise: a third of all pairs in reach, i.e. whole blocks inside the cutoff)


@pytest.mark.parametrize("restraints", [False, True], ids=["free", "restrained"])
@pytest.mark.parametrize("n_rec,n_lig,k_rec,k_lig", [(65, 63, 0, 10), (200, 130, 10, 10), (513, 65, 7, 1)])
def test_oracle_sums_on_the_flexing_random_molecules(orc, tmp_path, n_rec, n_lig, k_rec, k_lig, restraints):
    _check_constant_tables(T.random_anm_case(tmp_path, n_rec, n_lig, k_rec, k_lig, restraints), orc)


@pytest.mark.parametrize("n_lig", [64, 130])
@pytest.mark.parametrize("n_rec", T.BALL_SIZES)
def test_oracle_sums_and_extra_bits_of_the_ball(pkg, orc, tmp_path, n_rec, n_lig):
    """Every pair of the ball inside the cutoff, the sums exact, and `dfire_bm_fix_scale` takes the bits off that the GPU test
    is there for: x = 0 up to 8191 atoms within reach of a tile, 1 up to 16382, 2 from 16383."""
    case = T.ball_case(tmp_path, n_rec, n_lig)
    _check_constant_tables(case, orc, all_pairs=n_rec * n_lig)
    _check_dyadic(case, orc, T.ladder_table(10.0, 20, case.used(orc)), 20)
    xyz = case.cpu(orc, np.zeros(T.TABLE_LEN)).model(0)["coordinates"]
    assert len(np.unique(xyz, axis=0)) == n_rec and np.all((xyz ** 2).sum(1) <= 64.0)
    for vmax, e in ((1024.0, 10), (10.0, 4)):
        count, extra, scale = pkg.dfire_bm_fix_scale(xyz, 15.0 + 3.0, vmax)
        assert (count, extra, scale) == (n_rec, T.BALL_EXTRA_BITS[n_rec], 2.0 ** (44 - e - T.BALL_EXTRA_BITS[n_rec]))
        assert 20 <= 44 - e - extra                                   # g = 20 of the ladder table stays exact
        assert 64 * ((count + (1 << extra) - 1) >> extra) * 2 ** 44 < 2 ** 63


def test_oracle_sums_on_the_restrained_ball(orc, tmp_path):
    case = T.ball_case(tmp_path, 2000, 130, restraints=True)
    stats = _check_constant_tables(case, orc, all_pairs=2000 * 130)
    assert np.all(stats[:, 2] > 0) and np.all(stats[:, 3] > 0)     # the restraints are met: both products of the tail are live


def test_fixed_point_scale_over_the_magnitude_ladder(pkg, orc):
    """2^(44 - e), 2^e >= max(vmax, 1): e = 0 for a table far below 1 and for vmax == 1, vmax == 2^e stays, one ulp of the table's
    grid above it moves on; 1024 is the last value taken."""
    case = T.fixture_case("1ppe", orc)
    xyz = case.cpu(orc, np.zeros(T.TABLE_LEN)).model(0)["coordinates"]
    for vmax, g, e in T.LADDER:
        table = T.ladder_table(vmax, g, case.used(orc))
        assert pkg.dfire_bm_fix_scale(xyz, 24.0, float(np.abs(table).max())) == (len(xyz), 0, 2.0 ** (44 - e))
    assert [e for _, _, e in T.LADDER] == [0, 0, 1, 4, 4, 5, 10]
    for vmax in (np.nextafter(1024.0, np.inf), np.inf):
        assert pkg.dfire_bm_fix_scale(xyz, 24.0, float(vmax))[2] == 0.0
    with pytest.raises(pkg.LightdockError, match="table maximum"):      # (a NaN is no maximum: the C ABI refuses it; `bm_accepts` meets the entry itself)
        pkg.dfire_bm_fix_scale(xyz, 24.0, float("nan"))


def test_the_reference_arithmetic_of_the_gpu_tests():
    """fits_53_bits, isum and the tolerance unit on known values."""
    assert T.fits_53_bits(0) and T.fits_53_bits(2 ** 53 - 1) and T.fits_53_bits((2 ** 53 - 1) << 9) and not T.fits_53_bits(2 ** 53 + 1)
    assert T.fits_53_bits(-(8191 * 130) << 44) and not T.fits_53_bits(-(2 ** 60 + 1))
    big = np.full(3000, 2 ** 52, dtype=np.int64)
    assert T.isum(big) == 3000 * 2 ** 52 and T.isum(-big) == -3000 * 2 ** 52 and T.isum(big[:0]) == 0
    assert T.tail_bound(0.0) == 3.0 * 4.7 + 999.0 and T.tail_bound(-1e6) == 3.0 * (1e6 * 0.0157) + 999.0
    assert T.tail(0.0, np.zeros(8)) == 4.7
