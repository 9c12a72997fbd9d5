"""The small-angle scattering rule (ld_complex_saxs, lightdock-rust_amd/saxs.py) on the CPU: the library's
host-only entry points (form factors, sinc, fit) against the numpy restatement of tests/saxs_reference.py, the restatement
pinned on the figures of the rule's text, and saxs.py's curve parser, bin plan and size measures on made-up input."""
import ctypes
import math

import numpy as np
import pytest

import saxs_reference as sx
from test_analysis_cpu import tool_module

Q = np.concatenate([[0.0, 1e-9, 0.001], np.linspace(0.01, 1.0, 34)])


def close(got, want):
    """|delta| <= 1e-12 (1 + |value|): libm against libm differs by about 1e-16, a wrong digit of the table by 1e-7 at least."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool((np.abs(got - want) <= 1e-12 * (1.0 + np.abs(want))).all())


# ---- the tables -------------------------------------------------------------------------------------------------

def test_form_factors_against_the_restatement(pkg):
    got = pkg.saxs_form_factors(Q)
    assert got.shape == (len(Q), 6) and close(got, sx.form_factors(Q))


def test_the_table_sums_to_the_atomic_numbers(pkg):
    f0 = pkg.saxs_form_factors([0.0])[0]
    for e, z in enumerate(sx.Z):
        a, b, c, V = sx.TABLE[e]
        assert abs(sum(a) + c - z) < 0.01
        assert abs(f0[e] + sx.RHO0 * V - z) < 0.01
        assert abs(sx.form_factor(e, 0.0) + sx.RHO0 * V - z) < 0.01


def test_sinc_against_the_restatement(pkg):
    for w, bins in ((500, 64), (100, 7), (2000, 1024), (137, 33)):
        got = pkg.saxs_sinc(Q, w / 1000.0, bins)
        assert close(got, sx.sinc(Q, w, bins))
        assert (got[0] == 1.0).all()                      # x == 0
    r0 = 0.25
    assert pkg.saxs_sinc([0.4], 0.5, 1)[0, 0] == math.sin(0.4 * r0) / (0.4 * r0)


def test_table_refusals(pkg):
    lib = pkg.load_library()
    out = np.full(6 * 4, 7.0)
    p = out.ctypes.data_as(ctypes.c_void_p)

    def q_of(values):
        a = np.array(values, dtype=np.float64)
        return a, a.ctypes.data_as(ctypes.c_void_p)

    for bad in ([-1e-9], [1.0000001], [float("nan")], [float("inf")], [0.1, -0.2]):
        a, qp = q_of(bad)
        assert lib.ld_saxs_form_factors(qp, len(a), p) == -1
        assert lib.ld_saxs_sinc(qp, len(a), 500, 2, p) == -1
    a, qp = q_of([0.1])
    assert lib.ld_saxs_form_factors(qp, 0, p) == -1 and lib.ld_saxs_form_factors(qp, 1025, p) == -1
    assert lib.ld_saxs_form_factors(None, 1, p) == -1 and lib.ld_saxs_form_factors(qp, 1, None) == -1
    for width, bins in ((99, 2), (2001, 2), (500, 0), (500, 1025)):
        assert lib.ld_saxs_sinc(qp, 1, width, bins, p) == -1
    assert (out == 7.0).all()
    assert lib.ld_saxs_sinc(qp, 1, 100, 4, p) == 0 and lib.ld_saxs_sinc(qp, 1, 2000, 4, p) == 0


# ---- classes and pair classes -----------------------------------------------------------------------------------

def record(name, resname, element, short=False):
    line = "ATOM      1 %-4s %3s A   1    %8.3f%8.3f%8.3f" % (name, resname, 1.0, 2.0, 3.0)
    return line if short else line + "  1.00  0.00          %2s  " % element


def test_classes_of_records():
    want = ((record("CA", "GLY", " C"), 1), (record("N", "GLY", "N "), 2), (record("O", "HOH", " O"), 3), (record("P", "DA", " P"), 4),
            (record("SG", "CYS", " S"), 5), (record("H", "GLY", " H"), 0), (record("D1", "GLY", " D"), 0), (record("1HB", "ALA", ""), 0),
            (record("CA", "GLY", "", short=True), 1), (record("NZ", "LYS", ""), 2), (record("ZN", "ZN", "ZN"), 255), (record("CA", "CA", "CA"), 255),
            (record("SE", "MSE", "se"), 255), (record("BJ", "MMB", " C"), 255), (record("CL", "CL", "Cl"), 255), (record("od1", "ASP", " o"), 3))
    for line, e in want:
        assert sx.record_class(line) == e, line
    assert len(record("CA", "GLY", "", short=True)) == 54


def test_pair_classes():
    assert [sx.pair_class(0, f) for f in range(6)] == [0, 1, 2, 3, 4, 5]
    assert sx.pair_class(5, 5) == 20 and sx.pair_class(1, 1) == 6 and sx.pair_class(4, 5) == 19
    assert sorted({sx.pair_class(e, f) for e in range(6) for f in range(6)}) == list(range(21))
    assert all(sx.pair_class(e, f) == sx.pair_class(f, e) for e in range(6) for f in range(6))


def test_the_restated_histogram_on_pins():
    t = np.array([[0, 0, 0], [300, 400, 0], [299, 400, 0], [0, 0, 999], [5, 5, 5]])
    h = sx.histogram(t, np.array([1, 1, 3, 255, 0]), 500, 4)
    # C-C at exactly 500 -> bin 1; C-O at 499.4 -> bin 0; C-O 1 apart and every pair of the H: bin 0
    assert h[sx.pair_class(1, 1)].tolist() == [0, 1, 0, 0] and h[sx.pair_class(1, 3)].tolist() == [2, 0, 0, 0]
    assert h[sx.pair_class(0, 1)].tolist() == [2, 0, 0, 0] and h[sx.pair_class(0, 3), 0] == 1 and h.sum() == 6
    with pytest.raises(ValueError):
        sx.histogram(np.array([[0, 0, 0], [2000, 0, 0]]), np.array([1, 1]), 500, 4)
    assert sx.histogram(np.array([[0, 0, 0], [1999, 0, 0]]), np.array([1, 1]), 500, 4)[6, 3] == 1
    big = np.array([7264831, 94906267], dtype=np.int64)          # sqrt(3) 2^22, and near sqrt(2^53)
    assert sx.isqrt(big * big).tolist() == big.tolist() and sx.isqrt(big * big - 1).tolist() == (big - 1).tolist()


# ---- the fit ----------------------------------------------------------------------------------------------------

def test_fit_is_the_sequential_sums_exactly(pkg):
    rng = np.random.default_rng(3)
    n_q = 37
    i_exp = np.exp(rng.normal(8, 2, n_q))
    sigma = 0.03 * i_exp + 1e-3
    intensity = np.stack([i_exp * 2.5, i_exp * rng.uniform(0.5, 2.0, n_q), np.exp(rng.normal(3, 1, n_q)), -i_exp])
    scale, chi2 = pkg.saxs_fit(intensity, i_exp, sigma)
    for i in range(len(intensity)):
        s, c = sx.fit(intensity[i], i_exp, sigma)
        assert scale[i] == s and chi2[i] == c
    assert abs(scale[0] - 0.4) < 1e-12 and chi2[0] < 1e-20 and scale[3] < 0
    one = pkg.saxs_fit(intensity[:1, :1], i_exp[:1], sigma[:1])
    assert one[0][0] == sx.fit(intensity[0, :1], i_exp[:1], sigma[:1])[0]


def test_fit_refusals(pkg):
    lib = pkg.load_library()
    i_exp, sigma, intensity = np.array([1.0, 2.0, 3.0]), np.array([0.1, 0.1, 0.1]), np.array([[1.0, 2.0, 3.0], [2.0, 2.0, 2.0]])

    def call(intensity, i_exp, sigma, n=None, n_q=None):
        scale, chi2 = np.full(2, 7.0), np.full(2, 7.0)
        arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (intensity, i_exp, sigma)]
        status = lib.ld_saxs_fit(len(arrays[0]) if n is None else n, len(arrays[1]) if n_q is None else n_q,
                                 *[a.ctypes.data_as(ctypes.c_void_p) for a in arrays + [scale, chi2]])
        return status, bool((scale == 7.0).all() and (chi2 == 7.0).all())

    assert call(intensity, i_exp, sigma) == (0, False)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        s = sigma.copy()
        s[1] = bad
        assert call(intensity, i_exp, s) == (-1, True)
    zero = intensity.copy()
    zero[1] = 0.0                                           # the second pose: a zero denominator; nothing of the first is written
    assert call(zero, i_exp, sigma) == (-1, True)
    nan = intensity.copy()
    nan[0, 2] = float("nan")
    assert call(nan, i_exp, sigma) == (-1, True)
    assert call(intensity, [1.0, float("inf"), 3.0], sigma) == (-1, True)
    assert call(intensity, i_exp, sigma, n_q=0) == (-1, True) and call(intensity, i_exp, sigma, n=0) == (0, True)
    with pytest.raises(pkg.LightdockError):
        pkg.saxs_fit(zero, i_exp, sigma)


# ---- the Debye restatement on two atoms -------------------------------------------------------------------------

def test_restated_debye_of_two_atoms():
    q = np.array([0.0, 0.1, 0.33])
    f, s = sx.form_factors(q), sx.sinc(q, 500, 16)
    counts = np.zeros((21, 16), dtype=np.int64)
    counts[sx.pair_class(1, 3), 7] = 1
    got = sx.debye(counts, [0, 1, 0, 1, 0, 0], f, s)
    for j in range(3):
        assert got[j] == (0.0 + 1.0 * (f[j, 1] * f[j, 1]) + 1.0 * (f[j, 3] * f[j, 3])) + ((2.0 * f[j, 1]) * f[j, 3]) * (0.0 + 1.0 * s[j, 7])
    assert abs(got[0] - (f[0, 1] + f[0, 3]) ** 2) < 1e-9


# ---- saxs.py ----------------------------------------------------------------------------------------------------

def test_curve_parser():
    tool = tool_module("saxs")
    text = "# q I sigma\n\n0.01 100.0 3.0\n  0.02\t90 2.7  \n#0.025 1 1\n0.5 10 0.3\n0.6 5 0.2\n"
    q, i, s = tool.parse_curve(text)
    assert q.tolist() == [0.01, 0.02, 0.5] and i.tolist() == [100.0, 90.0, 10.0] and s.tolist() == [3.0, 2.7, 0.3]
    assert tool.parse_curve(text, qmax=1.0)[0].tolist() == [0.01, 0.02, 0.5, 0.6]
    nm = tool.parse_curve("0.1 100 3\n0.2 90 2.7\n6 5 1\n", unit="nm")
    assert nm[0].tolist() == [0.1 / 10.0, 0.2 / 10.0] and nm[1].tolist() == [100.0, 90.0]
    for bad in ("0.01 100\n", "0.01 100 3 4\n", "0.01 abc 3\n", "q I sigma\n", "0.02 1 1\n0.02 1 1\n", "0.02 1 1\n0.01 1 1\n",
                "0.01 1 0\n", "0.01 1 -1\n", "0.01 nan 1\n", "0.01 1 inf\n", "-0.01 1 1\n", "", "# only\n", "0.7 1 1\n"):
        with pytest.raises(ValueError):
            tool.parse_curve(bad)
    with pytest.raises(ValueError):
        tool.parse_curve("0.01 1 1\n", unit="cm")
    with pytest.raises(ValueError):
        tool.parse_curve("".join("%.6f 1 1\n" % (1e-4 * (k + 1)) for k in range(1025)))


def test_bin_plan():
    tool = tool_module("saxs")
    assert tool.bin_plan(100.0, 500) == (500, 201)          # 100 001 thousandths: 200 bins hold 100 000
    assert tool.bin_plan(511.9, 500) == (500, 1024)
    w, bins = tool.bin_plan(600.0, 500)
    assert w == 586 and bins <= 1024 and w * bins > 600000
    assert tool.bin_plan(0.0, 500) == (500, 1)
    with pytest.raises(ValueError):
        tool.bin_plan(2100.0, 500)
    assert tool.distance_bound(30.0, 10.0, np.array([[3.0, 4.0, 0.0, 1, 0, 0, 0]])) == 60.0 + tool.MODE_MARGIN
    assert tool.distance_bound(30.0, 10.0, np.array([[30.0, 40.0, 0.0, 1, 0, 0, 0]])) == 90.0 + tool.MODE_MARGIN


def test_size_measures_from_synthetic_counts():
    tool = tool_module("saxs")
    counts = np.zeros((21, 8), dtype=np.uint32)
    assert tool.size_measures(counts, 500, 1) == (0.0, 0.0)
    counts[6, 3] = 1                                        # two atoms, one pair in bin 3: r = 1.75 A
    rg, dmax = tool.size_measures(counts, 500, 2)
    assert rg == math.sqrt(1.75 ** 2 / 4.0) and dmax == 2.0
    counts[0, 0], counts[20, 5] = 2, 3
    rg, dmax = tool.size_measures(counts, 1000, 4)
    assert abs(rg - math.sqrt((2 * 0.5 ** 2 + 3.5 ** 2 + 3 * 5.5 ** 2) / 16.0)) < 1e-12 and dmax == 6.0


def test_rank_text_sorts_by_chi2_and_keeps_the_scoring_order_on_ties():
    tool = tool_module("saxs")
    entries = [(0, 5, None, {"scoring": 30.0}), (2, 1, None, {"scoring": 20.0}), (1, 7, None, {"scoring": 10.0})]
    chi2, scale = [2.0, 0.5, 2.0], [1.0, 2.0, 3.0]
    order = tool.rank_rows(entries, chi2)
    assert order == [1, 0, 2]
    lines = tool.rank_text(entries, order, chi2, scale, [(10.0, 30.0)] * 3).splitlines()
    assert lines[0].split() == ["Swarm", "Glowworm", "Scoring", "chi2", "scale", "Rg", "Dmax"]
    assert [l.split()[:2] for l in lines[1:]] == [["2", "1"], ["0", "5"], ["1", "7"]]
    assert lines[1].split()[3:] == ["5.000000e-01", "2.000000e+00", "10.000", "30.000"]
