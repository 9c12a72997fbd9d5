"""The cases of tests/assess_edges.py are what they say, on the CPU: the kappa of every rung, the exact degeneracies, the
integer distances of the tile cases, the aliasing property of every distance, the posed thousandths integers by construction;
reference_measures against test_assess_cpu.exact_fit; and an independent f64 method (numpy's eigh of Horn's matrix for
i-RMSD^2, test_assess_cpu.svd_lrmsd for L-RMSD^2) inside the bounds the GPU is held to, on every case that has one -- the
bounds are attainable by the reference side alone.  Nothing here runs the code under test."""
import decimal

import numpy as np
import pytest

import assess_edges as ae
from test_assess_cpu import EPS, det3, det4, exact_fit, exact_sums, fast_thousandths, svd_lrmsd
from test_contacts_cpu import thousandths


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    return str(tmp_path_factory.mktemp("assess_edges"))


def sets_of(b, k):
    rs, t = b.rs, b.case.model_thousandths(k)
    return (t[rs.rec_fit], rs.ref_t[rs.rec_fit], t[rs.lig_fit], rs.ref_t[rs.lig_fit], t[rs.interface_fit], rs.ref_t[rs.interface_fit])


def unique_poses(case):
    seen = {}
    for k, p in enumerate(case.poses):
        seen.setdefault(p, k)
    return sorted(seen.values())


def test_a_field_prints_its_thousandths_exactly():
    assert ae.field(-999999) == "-999.999" and ae.field(9999999) == "9999.999" and ae.field(1) == "   0.001"
    assert ae.field(-1990000) == "-1990.00" and ae.field(-1999990) == "-1999.99" and ae.field(-1000000) == "-1000.00"
    with pytest.raises(AssertionError):
        ae.field(-1990001)
    line = ae.atom_line(7, ae.atom("1HB", "LYS", "A", 12, (-1990000, 5, 1999999)))
    assert line[12:16] == "1HB " and (float(line[30:38]), float(line[38:46]), float(line[46:54])) == (-1990.0, 0.005, 1999.999)
    assert ae.atom_line(7, ae.atom("CA", "LYS", "A", 12, (0, 0, 0)))[12:16] == " CA "


def test_posed_thousandths_are_the_integers_of_the_construction(directory):
    """The f64 posing of the restatement (the device's arithmetic) prints the integers the cases are built of."""
    for case in ae.all_cases():
        b = ae.built(case, directory)
        rows = case.rows
        for k in unique_poses(case):
            assert np.array_equal(b.rs.posed_thousandths(rows[k])[b.rs.used], case.model_thousandths(k)[b.rs.used]), (case.name, k)
            assert np.abs(case.model_thousandths(k)[b.rs.used]).max() <= 2000000, case.name


def test_reference_measures_against_exact_fit(directory):
    """i-RMSD^2: the f64 of exact_fit's, and n lambda a root of exact_fit's integer quartic to 1e-40 of its scale (the Decimal
    inside exact_fit is not returned; this is the equation it solves).  The G's are exact_fit's."""
    D = decimal.Decimal
    worst = 0.0
    for case in ae.all_cases():
        b = ae.built(case, directory)
        for k in unique_poses(case)[:2]:
            m_int, r_int = sets_of(b, k)[4:]
            m = b.measures(k)
            i2, ga, gb = exact_fit(m_int, r_int)
            scale = (ga + gb) / len(m_int)
            assert m["ga"] == ga and m["gb"] == gb and m["n_int"] == len(m_int)
            assert abs(m["irmsd2"] - i2) <= 4 * EPS * scale, (case.name, m["irmsd2"], i2)
            n, A, B, K = exact_sums(m_int, r_int)
            with decimal.localcontext() as ctx:
                ctx.prec = 80
                N = ae.horn(K)
                c2, c1, c0 = D(-2 * sum(v * v for row in K for v in row)), D(-8 * det3(K)), D(det4(N))
                x, top = D(m["lambda_int"]), D(A + B) / 2
                residual = abs(((x * x + c2) * x + c1) * x + c0)
                assert x <= top * (1 + D(10) ** -40)
                if top > 0:
                    worst = max(worst, float(residual / top ** 4))
                    assert residual <= top ** 4 * D(10) ** -40, (case.name, residual / top ** 4)
    print("largest residual of the quartic at n lambda, over ((A + B) / 2)^4: %.1e" % worst)


# ---- solver cases ------------------------------------------------------------------------------------------------

def test_the_kappa_of_every_rung(directory):
    for width in ae.LADDER_WIDTHS:
        case = ae.ladder_case(width)
        m = ae.built(case, directory).measures(0)
        assert abs(m["kappa"] / case.expect["kappa"] - 1.0) < 0.01, (width, m["kappa"])
        assert m["lrmsd2"] > 0.01 and m["irmsd2"] > 0.01                       # no rung is a perfect fit
        print("width %4d: kappa %.4g, lambdas %s" % (width, m["kappa"], m["lambdas"]))
    kappas = [ae.built(ae.ladder_case(w), directory).measures(0)["kappa"] for w in ae.LADDER_WIDTHS]
    assert 50 < kappas[0] < 200 and all(90 < b / a < 110 for a, b in zip(kappas, kappas[1:])) and kappas[3] > 5e7


def minors_vanish(K):
    return all(K[a][b] * K[c][d] == K[a][d] * K[c][b] for a in range(3) for c in range(3) for b in range(3) for d in range(3))


def test_exact_degeneracies(directory):
    """Width 0 and the collinear interface: n S has rank 1 in exact integers, so Horn's eigenvalues are s, s, -s, -s; S = 0: all
    four are 0.  mpmath agrees to 60 digits."""
    import mpmath
    b = ae.built(ae.ladder_case(0), directory)
    sets = sets_of(b, 0)
    K = exact_sums(sets[0], sets[1])[3]
    assert minors_vanish(K) and any(v for row in K for v in row)
    m = b.measures(0)
    assert np.isinf(m["kappa"]) and ae.bounds(m)[1] is None and m["lambdas"][0] == m["lambdas"][1] == 1.0
    with mpmath.workdps(ae.DIGITS):
        lam = ae.spectrum(sets[0], sets[1])[3]
        assert abs(lam[0] - lam[1]) <= abs(lam[0]) * mpmath.mpf(10) ** -55 and lam[0] > 0
    K = exact_sums(sets[4], sets[5])[3]
    assert not minors_vanish(K)                                               # its interface set is not collinear
    assert np.isfinite(ae.lrmsd_cap(m)) and 0 <= m["lrmsd2"] <= ae.lrmsd_cap(m)

    b = ae.built(ae.collinear_interface_case(), directory)
    sets = sets_of(b, 0)
    K = exact_sums(sets[4], sets[5])[3]
    assert minors_vanish(K) and any(v for row in K for v in row)
    with mpmath.workdps(ae.DIGITS):
        lam = ae.spectrum(sets[4], sets[5])[3]
        assert abs(lam[0] - lam[1]) <= abs(lam[0]) * mpmath.mpf(10) ** -55 and lam[0] > 0
    centred = sets[5] * len(sets[5]) - sets[5].sum(axis=0)
    assert np.linalg.matrix_rank(centred.astype(float)) == 3                  # the reference's interface is not collinear
    assert np.isfinite(b.measures(0)["kappa"]) and b.measures(0)["kappa"] < 100

    b = ae.built(ae.zero_s_case(), directory)
    sets = sets_of(b, 0)
    n, A, B, K = exact_sums(sets[4], sets[5])
    assert n == 4 and not any(v for row in K for v in row) and A > 0 and B > 0
    m = b.measures(0)
    assert abs(m["irmsd2"] - (m["ga"] + m["gb"]) / 4) <= EPS * (m["ga"] + m["gb"])
    assert np.isfinite(m["kappa"])


def test_turned_and_mirrored_references(directory):
    for which in sorted(ae.TURNS):
        m = ae.built(ae.turned_case(which), directory).measures(0)
        assert m["irmsd2"] < 1e-6 and 0 < m["lrmsd2"] < 1e-5 and m["kappa"] < 10, which           # a fit but for the reprint's rounding
        q = np.abs(m["q"])
        if which.startswith("half"):
            assert q[0] < 1e-4 and q[1:].min() > 0.2 or which == "half_110" and q[1] > 0.7 and q[2] > 0.7, (which, q)
        else:
            assert q[0] > 1 - 1e-9 and 1e-8 < q[1:].max() < 1e-6, (which, q)
    off = [ae.built(ae.turned_case(k), directory).measures(0)["q"][0] for k in ("half_plus", "half_minus")]
    assert off[0] != 0.0 and off[1] != 0.0                                    # 0.001 degrees from the half turn, either side
    m = ae.built(ae.mirror_case(), directory).measures(0)
    assert m["irmsd2"] > 1.0 and m["lambdas"][3] == -1.0 and m["lambdas"][0] < 0.9                 # a mirror image is not a fit
    kappas = []
    for d in ae.MIRROR_D:
        b = ae.built(ae.mirror_family_case(d), directory)
        sets = sets_of(b, 0)
        K = exact_sums(sets[0], sets[1])[3]
        assert det3(K) < 0
        sv = np.linalg.svd(np.array(K, dtype=float), compute_uv=False)
        kappas.append(b.measures(0)["kappa"])
        print("mirror family d %4d: kappa %.4g, (s2 - s3) / s1 %.3g" % (d, kappas[-1], (sv[1] - sv[2]) / sv[0]))
        assert abs(kappas[-1] * 2 * (sv[1] - sv[2]) / sv.sum() - 1.0) < 1e-3
    assert kappas[0] < 10 < kappas[1] < 1000 < kappas[2]                       # every member kept: kappa grows as d shrinks


def test_large_sums_small_spreads(directory):
    m = ae.built(ae.perfect_far_case(), directory).measures(0)
    assert m["irmsd2"] == 0.0 and m["lrmsd2"] < 1e-100 and m["ga"] > 1e7 and m["gla"] > 1e7 and m["kept"] == 12

    case = ae.corner_case()
    b = ae.built(case, directory)
    t = case.model_thousandths(0)
    corner = np.array([1990000, -1990000, 1990000])
    assert np.sqrt(((t[:b.rs.n_rec] - corner) ** 2).sum(axis=1)).max() <= 5000.0
    assert np.abs(t[b.rs.n_rec:] - corner).max() <= 6000 and np.abs(t).max() < 2000000 and np.abs(t).min() > 1980000
    assert np.abs(b.rs.ref_t - np.array([-1500000, 1500000, -1500000])).max() < 12000
    m = b.measures(0)
    assert 0.1 < m["irmsd2"] < 3.0 and 0.1 < m["lrmsd2"] < 3.0 and m["ga"] < 300 and m["gla"] < 300 and m["kappa"] < 10
    assert sum(int(v) ** 2 for v in t[b.rs.rec_fit].ravel()) > 30 * 1985000 ** 2 > 1e5 * m["ga"] * 1e6       # the raw sum against the centred one

    case = ae.spread_case()
    b = ae.built(case, directory)
    assert b.rs.counts() == {"matched_rec": 4096, "matched_lig": 4096, "native_pairs": 1, "rec_fit": 4096, "lig_fit": 4096, "interface_fit": 8}
    t = case.model_thousandths(0)
    ss = sum(int(v) ** 2 for v in t[b.rs.rec_fit].ravel())
    assert 2 ** 53 < ss < 2 ** 55 and 2 ** 65 < 4096 * ss < 2 ** 67 and np.abs(t).max() <= 1990000
    m = b.measures(0)
    assert 2.0 < m["irmsd2"] < 6.0 and 3.0 < m["lrmsd2"] < 5.0 and m["ga"] > 1e7       # noise uniform in +-2 A: 4 A^2 in the mean


# ---- sums-kernel cases -------------------------------------------------------------------------------------------

def pair_distances(b, k, pair=0):
    t = b.case.model_thousandths(k)
    a, c = b.rs.pair_atoms[pair]
    d = t[a][:, None, :] - t[c][None, :, :]
    return (d * d).sum(axis=2)


@pytest.mark.parametrize("corner", ae.TILE_CORNERS)
def test_tile_cases(directory, corner):
    for case in ae.tile_cases(corner):
        n_rec, n_lig, _ = case.expect["tile"]
        b = ae.built(case, directory)
        assert b.rs.native == [(0, 0)] and b.rs.counts()["native_pairs"] == 1
        assert (len(b.rs.pair_atoms[0][0]), len(b.rs.pair_atoms[0][1])) == (n_rec, n_lig)
        d2 = pair_distances(b, 0)
        at = (0 if corner.startswith("first") else n_rec - 1, 0 if corner.endswith("first") else n_lig - 1)
        t = case.model_thousandths(0)
        assert d2[at] == 5000 ** 2 and tuple(t[b.rs.pair_atoms[0][1][at[1]]] - t[b.rs.pair_atoms[0][0][at[0]]]) == (3000, 4000, 0)
        others = np.delete(d2.ravel(), at[0] * n_lig + at[1])
        assert len(others) == n_rec * n_lig - 1 and (len(others) == 0 or others.min() == 5500 ** 2)
        d2 = pair_distances(b, 1)
        assert d2[at] == 3001 ** 2 + 4000 ** 2 == d2.min() == 25006001
        assert [b.measures(k)["kept"] for k in (0, 1)] == [1, 0]
    # hydrogens and atoms that are no fit atoms fill the residues up
    big = ae.built(ae.tile_case(24, 24, corner), directory).rs
    assert big.used[:24].all() and int(big.fit[:24].sum()) == 4 and big.counts()["rec_fit"] == 8
    slot = ae.slot_case()
    assert len(slot.poses) == 1030 > 1024 and slot.poses[:3] == [(0, 0, 0), (1, 0, 0), (0, 0, 0)] and slot.expect["tile"] == (17, 9, "last_last")


def test_pair_count_cutoff_and_aliasing_cases(directory):
    for count in ae.PAIR_COUNTS:
        case = ae.pairs_case(count)
        b = ae.built(case, directory)
        assert len(b.rs.native) == count == b.rs.counts()["native_pairs"]
        assert [b.measures(k)["kept"] for k in range(4)] == case.expect["kept"] == [count, 0, (count + 1) // 2, count // 2]
        for i in range(count):
            assert pair_distances(b, 0, i).min() == 5000 ** 2 and np.sort(pair_distances(b, 0, i).ravel())[1] == 5500 ** 2
    for C in (1, 30000):
        case = ae.cutoff_case(C)
        b = ae.built(case, directory)
        extra = len(b.rs.native) - 1                       # at C = 30000 the anchors are a native pair too, always kept
        assert extra == (1 if C == 30000 else 0) and b.rs.native[0] == (0, 0)
        assert [b.measures(k)["kept"] - extra for k in range(4)] == case.expect["kept_of_pair"]
        assert [int(pair_distances(b, k).min()) for k in range(4)] == [C * C, C * C + 1, (C + 1) ** 2, (C - 1) ** 2]
    case = ae.aliasing_case()
    single, triple = case.expect["distances"]
    assert len(single) == 3 and len(set(single)) == 3 and len(set(triple)) == 3
    for d in single:
        assert 65536 <= d <= 3999800 and (d * d) % 2 ** 32 <= 5000 ** 2 < d * d
    assert all(65536 <= d <= 3999800 for d in triple) and sum(d * d for d in triple) % 2 ** 32 <= 5000 ** 2
    assert sum((d * d) % 2 ** 32 for d in triple) <= 5000 ** 2
    b = ae.built(case, directory)
    assert len(b.rs.native) == 1
    assert [b.measures(k)["kept"] for k in range(5)] == case.expect["kept"] == [1, 0, 0, 0, 0]
    for k, want in enumerate([(3000, 0, 0)] + [(d, 0, 0) for d in single] + [triple]):
        t = case.model_thousandths(k)
        assert tuple(t[b.rs.pair_atoms[0][1][0]] - t[b.rs.pair_atoms[0][0][0]]) == want
        if k:
            assert int(pair_distances(b, k).astype(object).min()) > 32767 ** 2       # every atom pair of the two residues past the clamp


def test_used_atom_cases(directory):
    for n_rec_used, n_lig_used in ae.USED_COUNTS:
        b = ae.built(ae.used_case(n_rec_used, n_lig_used), directory)
        rs = b.rs
        side = np.arange(len(rs.used)) >= rs.n_rec
        assert (int((rs.used & ~side).sum()), int((rs.used & side).sum())) == (n_rec_used, n_lig_used)
        kinds = {"unmatched": ~rs.matched, "unused": rs.matched & ~rs.used, "used, no fit atom": rs.used & ~rs.fit,
                 "fit outside": rs.fit & ~rs.interface_fit, "interface fit": rs.interface_fit}
        for mask, n_used in ((~side, n_rec_used), (side, n_lig_used)):
            present = {k for k, v in kinds.items() if (v & mask).any()}
            missing = set(kinds) - present
            allowed = {"unused", "fit outside"} | ({"used, no fit atom"} if n_used in (1, 3) else set())      # a side of 1 or 3 used atoms
            assert missing <= allowed and (n_used > 4 or missing), (n_rec_used, n_lig_used, missing)
            if n_used > 4:
                assert not missing
                order = np.flatnonzero(mask)
                label = np.array([[k for k, v in kinds.items() if v[i]][0] for i in order])
                assert (label[1:] != label[:-1]).sum() > n_used                # interleaved, not in blocks
        assert len(rs.native) == 1 and b.measures(0)["irmsd2"] > 1e-3


def test_the_coordinate_bound_case(directory):
    case = ae.bound_case()
    b = ae.built(case, directory)
    rs = b.rs
    lig_used = np.flatnonzero(rs.used[rs.n_rec:]) + rs.n_rec
    assert len(lig_used) == 4
    extremes = [(case.model_thousandths(k)[lig_used].max(), case.model_thousandths(k)[lig_used].min()) for k in range(4)]
    assert [e[0] for e in extremes[::2]] == [2000000, 2000000] and [e[1] for e in extremes[1::2]] == [-2000000, -2000000]
    far = ae.xyz_of(case.lig)
    assert (~rs.matched[rs.n_rec:] & (far[:, 0] == 5000000)).sum() == 1                            # unmatched, at 5000 A
    assert (rs.matched[rs.n_rec:] & ~rs.used[rs.n_rec:] & (far[:, 0] == 4000000)).sum() == 1       # matched, unused, at 4000 A
    for row in ae.REFUSED_ROWS:
        t = fast_thousandths(rs.pose(row)[lig_used])
        assert np.abs(t).max() in (2000001,) and np.array_equal(t, thousandths(rs.pose(row)[lig_used]))
    for row, k in zip(ae.ACCEPTED_ROWS, (0, 3)):
        assert np.array_equal(fast_thousandths(rs.pose(row))[rs.used], case.model_thousandths(k)[rs.used])
    assert [b.measures(k)["kept"] for k in range(5)] == [0, 0, 0, 0, 1]


# ---- the bounds are attainable -----------------------------------------------------------------------------------

def eigh_irmsd2(m, r):
    """i-RMSD^2 in A^2 by numpy's eigh of Horn's matrix in f64, the sets centred on their integer-rounded centroids first."""
    cm, cr = np.rint(m.mean(axis=0)).astype(np.int64), np.rint(r.mean(axis=0)).astype(np.int64)
    P, Q = (m - cm) / 1000.0, (r - cr) / 1000.0
    P, Q = P - P.mean(axis=0), Q - Q.mean(axis=0)
    lam = np.linalg.eigvalsh(np.array(ae.horn((P.T @ Q).tolist())))[-1]
    return ((P * P).sum() + (Q * Q).sum() - 2.0 * lam) / len(P)


def test_an_independent_f64_method_stays_inside_the_bounds(directory):
    """numpy's eigh and SVD, not the code under test: what the bounds ask is within reach of f64."""
    worst = {"irmsd": (0.0, None), "lrmsd": (0.0, None)}
    unspecified = 0
    for case in ae.all_cases():
        b = ae.built(case, directory)
        for k in unique_poses(case):
            sets, m = sets_of(b, k), b.measures(k)
            bi, bl = ae.bounds(m)
            di = abs(eigh_irmsd2(sets[4], sets[5]) - m["irmsd2"])
            worst["irmsd"] = max(worst["irmsd"], (di / (bi / 64), case.name))
            assert di <= bi, (case.name, k, di / (bi / 64))
            l2, gla, glb = svd_lrmsd(*sets[:4])
            assert abs(gla - m["gla"]) <= 8 * EPS * m["gla"] and abs(glb - m["glb"]) <= 8 * EPS * m["glb"]
            if bl is None:
                unspecified += 1
                assert 0.0 <= l2 <= ae.lrmsd_cap(m)
                continue
            dl = abs(l2 - m["lrmsd2"])
            worst["lrmsd"] = max(worst["lrmsd"], (dl / (bl / 128), case.name))
            assert dl <= bl, (case.name, k, dl / (bl / 128), m["kappa"])
    assert unspecified == 1
    print("numpy against the 60-digit reference, worst ratios: i-RMSD^2 %.3f of eps G / n (%s), L-RMSD^2 %.3f of eps G / n_l (1 + kappa) (%s)"
          % (worst["irmsd"] + worst["lrmsd"]))
