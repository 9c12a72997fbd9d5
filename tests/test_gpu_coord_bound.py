"""The one coordinate bound of the analysis kernels on the MI355X (kComplexCoordBound of kernels/complex_rule.hpp, 10^9
thousandths): every call that poses with it, at the bound itself and one thousandth beyond, on each axis and sign.

A one-atom receptor at the origin and a one-atom ligand, no modes; the pose translates the ligand to +-1 000 000.000 A (accepted,
equal to the numpy restatement of that call) and to +-1 000 000.001 A (refused with the call's overflow message, the outputs
untouched).  So that the bound decides and no other limit of a call: the collision cross-section is the ligand's alone
(what = 1: the complex's box would exceed 2^28 lattice points), and the scattering's receptor is a zinc, which takes no part
(a pair 10^6 A long lies beyond every last bin)."""
import ctypes

import numpy as np
import pytest

import ccs_reference as cr
import emfit_reference as er
import fcc_reference as fr
import sasa_reference as sr
import saxs_reference as sx
from test_contacts_cpu import ContactsRestated, thousandths
from test_gpu_ccs import raw_call as raw_ccs
from test_gpu_emfit import raw_fit
from test_gpu_sasa import atom, pair_of_files, raw_call as raw_sasa, untouched

pytestmark = pytest.mark.gpu

BOUND = 10 ** 9
VP = ctypes.c_void_p
MARK32 = 0xA5A5A5A5
BEYOND = "a posed coordinate is beyond +-1.0e6 A"


def translated(x):
    """The six poses that put the ligand's atom at +-x on one axis: +x, -x, +y, -y, +z, -z."""
    poses = np.zeros((6, 7))
    poses[:, 3] = 1.0
    for k in range(3):
        poses[2 * k, k], poses[2 * k + 1, k] = x, -x
    return poses


AT, OVER = translated(1000000.0), translated(1000000.001)
NEAR = np.array([[3.0, -4.0, 0.0, 1.0, 0.0, 0.0, 0.0]])     # 5.000 A apart: a contact, so that an accepted batch is not all empty


def ptr(a):
    return a.ctypes.data_as(VP)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("bound")
    carbon = pair_of_files(d, atom(1, "C", "GLY", "A", 1, (0, 0, 0), "C"), atom(1, "C", "GLY", "B", 1, (0, 0, 0), "C"), "c")
    zinc = pair_of_files(d, atom(1, "ZN", "ZN", "A", 1, (0, 0, 0), "ZN", True), atom(1, "C", "GLY", "B", 1, (0, 0, 0), "C"), "zn")
    return carbon, zinc


@pytest.fixture(scope="module")
def carbons(pkg, files):
    pkg.init(0)
    return pkg.Complex(*files[0])


def refused(lib, status, message):
    assert status == -1 and lib.ld_last_error().decode() == message
    return True


def test_the_poses_are_the_bound_and_one_thousandth_beyond(files):
    rs = ContactsRestated(*files[0])
    for poses, want in ((AT, BOUND), (OVER, BOUND + 1)):
        for i, p in enumerate(poses):
            t = thousandths(rs.pose(p))
            expect = np.zeros((2, 3), dtype=np.int64)
            expect[1, i // 2] = want if i % 2 == 0 else -want
            assert np.array_equal(t, expect)


def test_contacts(pkg, carbons, files):
    lib, rs = pkg.load_library(), ContactsRestated(*files[0])
    poses = np.vstack([AT, NEAR])
    got = carbons.contacts(poses)
    want_rec, want_lig = rs.batch(poses)
    assert np.array_equal(got["rec"], want_rec) and np.array_equal(got["lig"], want_lig)
    assert [bool(v) for v in got["rec"][:, 0]] == [False] * 6 + [True]
    for p in OVER:
        batch = np.ascontiguousarray(np.vstack([NEAR, p[None], NEAR]))
        rec, lig = np.full((3, 1), MARK32, dtype=np.uint32), np.full((3, 1), MARK32, dtype=np.uint32)
        assert refused(lib, lib.ld_complex_contacts(carbons._h, 3, ptr(batch), 7, ctypes.c_double(5.0), ptr(rec), ptr(lig)), BEYOND)
        assert (rec == MARK32).all() and (lig == MARK32).all()


def test_pair_contacts_and_fcc_pair_sets(pkg, carbons, files):
    lib, rs = pkg.load_library(), ContactsRestated(*files[0])
    poses = np.vstack([AT, NEAR])
    offsets, keys = carbons.pair_contacts(poses)
    want = fr.pair_sets(rs, poses)
    assert np.array_equal(offsets.astype(np.int64), want[0]) and np.array_equal(keys.astype(np.int64), want[1])
    assert list(want[0]) == [0] * 7 + [1] and list(want[1]) == [0]
    for p in OVER:                                     # the sets of ld_complex_cluster_fcc are the same kernel's
        batch = np.ascontiguousarray(np.vstack([NEAR, p[None], NEAR]))
        o, k, total = np.full(4, MARK32, dtype=np.uint32), np.full(8, MARK32, dtype=np.uint32), ctypes.c_size_t(7)
        status = lib.ld_complex_pair_contacts(carbons._h, 3, ptr(batch), 7, ctypes.c_double(5.0), ptr(o), ptr(k), k.size, ctypes.byref(total))
        assert refused(lib, status, BEYOND) and (o == MARK32).all() and (k == MARK32).all() and total.value == 7
        cl, ce, nc = np.full(3, -7, dtype=np.int32), np.full(3, -7, dtype=np.int32), np.full(1, MARK32, dtype=np.uint32)
        s3 = np.zeros(3)
        status = lib.ld_complex_cluster_fcc(carbons._h, 3, ptr(batch), 7, ptr(s3), ctypes.c_double(5.0), ctypes.c_double(0.6), 1, ptr(cl), ptr(ce),
                                            ptr(nc), None, None)
        assert refused(lib, status, BEYOND) and (cl == -7).all() and (ce == -7).all() and nc[0] == MARK32


def test_sasa(pkg, carbons, files):
    lib, rs = pkg.load_library(), sr.SasaRestated(*files[0])
    poses = np.vstack([AT, NEAR])
    got = carbons.sasa(poses, atoms=True)
    sums, free, bound = rs.batch(poses)
    assert np.array_equal(got["sums"], sums) and np.array_equal(got["free"], free) and np.array_equal(got["bound"], bound)
    assert all(np.array_equal(free[i], bound[i]) for i in range(6)) and not np.array_equal(free[6], bound[6])
    for p in OVER:
        out = raw_sasa(lib, carbons, np.vstack([NEAR, p[None], NEAR]))
        assert refused(lib, out[0], BEYOND) and untouched(out[1:])


def test_saxs_with_a_receptor_that_takes_no_part(pkg, files):
    pkg.init(0)
    lib, cx, rs = pkg.load_library(), pkg.Complex(*files[1]), sx.SaxsRestated(*files[1])
    assert rs.n_part == 1 and list(cx.saxs_classes(0)) == [255]
    got = cx.distance_histogram(AT, 0.5, 8)
    assert got.shape == (6, 21, 8) and np.array_equal(got, rs.batch(AT, 500, 8)) and not got.any()
    message = "a pair of atoms lies beyond the last bin, or a posed coordinate beyond +-1.0e6 A"
    for p in OVER:
        batch = np.ascontiguousarray(np.vstack([AT[:1], p[None], AT[1:2]]))
        buf = np.full((3, 21, 8), MARK32, dtype=np.uint32)
        assert refused(lib, lib.ld_complex_distance_histogram(cx._h, 3, ptr(batch), 7, 500, 8, ptr(buf)), message)
        assert (buf == MARK32).all()


def test_density_fit(pkg, carbons, files):
    lib, rs = pkg.load_library(), er.EmfitRestated(*files[0])
    origin, step, sigma = (-2000, -2000, -2000), (1000, 1000, 1000), 300
    dens = pkg.Density(np.random.default_rng(4).normal(0.2, 1.0, (4, 4, 4)).astype(np.float32), origin, step)
    E = dens.voxels().astype(np.int64)
    poses = np.vstack([AT, NEAR])
    got = carbons.density_fit(poses, dens, sigma)
    want = [rs.fit(p, E, origin, step, sigma)[0] for p in poses]
    assert er.same_words(got, want)
    assert [w["outside"] for w in want] == [1] * 7 and want[0]["s"] > 0       # the receptor's atom is inside the map, the ligand's never
    message = "a simulated voxel reaches 2^24 or a pose's sum 2^40, or a posed coordinate lies beyond +-1.0e6 A"
    for p in OVER:
        status, clean = raw_fit(lib, carbons, dens, np.vstack([NEAR, p[None], NEAR]), sigma)
        assert refused(lib, status, message) and clean
        status, clean = raw_fit(lib, carbons, dens, p[None], sigma, simulate=True, voxels=64)
        assert refused(lib, status, message) and clean


def test_ccs_of_the_ligand_alone(pkg, carbons, files):
    lib, rs = pkg.load_library(), cr.CcsRestated(*files[0])
    got = carbons.ccs(AT, 1, 1.0, 0.5, views=True)
    counts, sums = rs.batch(AT, 1, 1.0, 0.5)
    assert np.array_equal(got["counts"], counts) and np.array_equal(got["sums"], sums) and counts.all()
    message = "a posed coordinate is beyond +-1.0e6 A, or a view's box holds more than 2^28 lattice points"
    for p in OVER:
        with pytest.raises(cr.Refused, match="beyond"):
            rs.ccs(p, 1)
        out = raw_ccs(lib, carbons, np.vstack([AT[:1], p[None], AT[1:2]]), what=1)
        assert refused(lib, out[0], message) and untouched(out[1:])
