"""Restraint and membrane flags of every pair route against the oracle at every slot layout of tests/flag_layouts.py (run with
-m gpu on an MI355X): which bit a pair sets -- the second and later flag words of either side, groups across a word boundary,
a side without words, every block tracked -- and what pose_energy_tail makes of the bits, membrane_beads at every entry and
exit of its four-trip loop included.  tests/test_flag_layouts_cpu.py holds, on the oracle alone, that the layouts realise all
that.

Per layout and route (tests/test_gpu_dfire_edges.py's ROUTES: the default, LIGHTDOCK_DFIRE_KERNEL=packed with
LIGHTDOCK_PACKED_CELLS 1 and 2, and allpairs; kernel_info()'s pair kernel is asserted, so a declined route does not pass as
the forced one) and per table:
  zero    potential = 0: the energy is a function of the flags alone and must equal the oracle's BIT FOR BIT (np.array_equal);
  synth   the seeded synthetic table, the markers sharing their blocks with real sums: test_gpu_parity.py's measures (bm_err on
          the block-major route, rel_err elsewhere) below its REL_TOL.  One hit is at least |score| / 98 of the energy and one
          bead 999 / 65, many orders above that.
all poses in one energy_batch, the same poses in reverse order (a pose's flag words must not leak into its neighbour's), the
counting launch (energies held to the same comparison, counts equal to the oracle's stats[5]), and Scorer.decompose's terms:
rec_restraints, lig_restraints and membrane equal to stats[2], stats[3], stats[4] exactly under both tables, its energy equal
to energy_batch's bits under the zero table and within the same measure of it under the synthetic one (decompose.hip sums a
pose's pairs in f64 in its own order; test_gpu_decompose.py compares the two the same way).

The default route on the zero table is `dfire_bm_pairs` for every layout, the ANM form included, as under the synthetic table:
the fixed-point scale is derived from max(|table|, 1), so a table maximum of 0 declines nothing (scorer.cpp:
dfire_bm_fix_scale), and every receptor subtile is quiet (bm_quiet_subtiles is asserted).

A failure prints the layout, the route, the pose's shift (a, b), the oracle's three hit counts and, under the zero table, the
counts that the GPU's energy implies.

DNA / PYDOCK (pose_energy_pairs<1, *>): the (33, 25, 58, 2) and (7, 32, 39, 1) lattices as arrays through Scorer.from_arrays,
the receptor in 3 and 2 chunks (LIGHTDOCK_CHUNK_ATOMS=64: flags of different chunks must OR together), against
dna_reference within its derived bound; one hit and one bead each exceed 100 x that bound on the compared poses.
"""
import numpy as np
import pytest

import flag_layouts as fl
from test_gpu_dfire_edges import BM, PACKED, ROUTES, _per_pose
from test_gpu_dna_pairs import build as build_dna, check_within_bound
from test_gpu_parity import REL_TOL, _counts_of, bm_err, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built(pkg, orc, table, tmp_path_factory):
    pkg.init(0)
    directory = str(tmp_path_factory.mktemp("flag_layouts"))
    return lambda name: fl.layout(orc, table, directory, name)


def _scorer(pkg, monkeypatch, g, which, route):
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    try:
        return pkg.Scorer.from_pdb("dfire", g.rec_pdb, g.lig_pdb, potential=g.tables[which], **g.kwargs)
    finally:
        for k in ROUTES[route]:
            monkeypatch.delenv(k)


def _explain(g, route, kernel, which, what, got, i):
    hr, hl, nb = g.hits(which)
    text = "%s, route %s (%s), table %s, %s: got %.17g, the oracle %.17g with hits (receptor %d of %d, ligand %d of %d, beads %d of %d)" % (
        g.label(i), route, kernel, which, what, got[i], g.energy[which][i], hr[i], g.n_rec_groups, hl[i], g.n_lig_groups, nb[i], g.n_beads)
    if which == "zero":
        text += "; the energy got implies (receptor, ligand, beads) = %s" % (g.counts_implied(got[i]) or "no counts at all")
    return text


def _hold(g, route, kernel, which, what, got, want=None):
    """Zero table: the bits.  Synthetic table: test_gpu_parity.py's measure of the route below REL_TOL."""
    want = g.energy[which] if want is None else want
    assert got.shape == want.shape
    if which == "zero":
        bad = np.flatnonzero(~((got == want) & (np.signbit(got) == np.signbit(want))))
        print("%s %s table zero %s: %d of %d poses differ in a bit" % (g.name, route, what, bad.size, len(want)))
        assert np.array_equal(got, want), "%d poses off, the first: %s" % (bad.size, _explain(g, route, kernel, which, what, got, bad[0]))
        return
    measure = bm_err if kernel == BM else rel_err
    per = _per_pose(got, want, kernel == BM)
    print("%s %s table synth %s: %s %.2e" % (g.name, route, what, measure.__name__, measure(got, want)))
    assert measure(got, want) < REL_TOL, "%d poses off, the worst: %s" % (
        int((per >= REL_TOL).sum()), _explain(g, route, kernel, which, what, got, int(np.argmax(per))))


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", list(fl.LAYOUTS))
def test_flags_against_the_oracle(built, pkg, monkeypatch, name, route):
    torch = pytest.importorskip("torch")
    g = built(name)
    poses = g.poses
    for which in ("zero", "synth"):
        hip = _scorer(pkg, monkeypatch, g, which, route)
        kernel = hip.kernel_info()["pair_kernel_name"]
        if route == "default":
            assert kernel == BM, (name, which, kernel)
            if which == "zero":
                assert hip.bm_quiet_subtiles() >= -(-len(g.rec_atoms) // 8), (name, hip.bm_quiet_subtiles())   # every subtile that holds an atom
        else:
            assert kernel == PACKED if route.startswith("packed") else kernel not in (BM, PACKED), (name, route, kernel)
        stats = g.stats[which]
        got = hip.energy_batch(poses)
        _hold(g, route, kernel, which, "energy_batch", got)
        _hold(g, route, kernel, which, "energy_batch in reverse order", hip.energy_batch(np.ascontiguousarray(poses[::-1]))[::-1])
        counted, counts = _counts_of(torch, hip, poses.copy())
        _hold(g, route, kernel, which, "counting launch", counted)
        off = np.flatnonzero(counts.astype(np.int64) != stats[:, 5].astype(np.int64))
        assert off.size == 0, "%s, route %s (%s), table %s: %d pairs counted, the oracle counts %d; %d poses off" % (
            g.label(off[0]), route, kernel, which, counts[off[0]], stats[off[0], 5], off.size)
        terms = hip.decompose(poses)["terms"]
        for key, column in (("rec_restraints", 2), ("lig_restraints", 3), ("membrane", 4)):
            bad = np.flatnonzero(terms[key] != stats[:, column])
            assert bad.size == 0, "decompose %s = %.17g, the oracle's fraction %.17g; %d poses off, the first: %s" % (
                key, terms[key][bad[0]], stats[bad[0], column], bad.size, _explain(g, route, kernel, which, "decompose", terms["energy"], bad[0]))
        _hold(g, route, kernel, which, "decompose energy", terms["energy"].copy(), want=None if which == "zero" else got)
        if which == "zero":
            assert np.array_equal(terms["energy"], got)


@pytest.mark.parametrize("method", ["dna", "pydock"])
@pytest.mark.parametrize("name", sorted(fl.DNA_LATTICES))
def test_dna_pairs_on_the_lattices(pkg, orc, monkeypatch, name, method):
    rec, lig, poses, shifts, want, shape = fl.dna_case(orc, name)
    n_rec_groups, n_lig_groups, n_membrane = len(rec["restraint_offsets"]) - 1, len(lig["restraint_offsets"]) - 1, len(rec["membrane"])
    assert shape[3] >= 2 and not any(w["nan"] for w in want)
    # the lattice reaches the edges of the counts here too: nothing, one, some and all of every term
    hr = {int(round(w["rec_restraints"] * n_rec_groups)) for w in want}
    hl = {int(round(w["lig_restraints"] * n_lig_groups)) for w in want}
    nb = {int(round(w["membrane"] * n_membrane)) for w in want}
    for seen, most in ((hr, n_rec_groups), (hl, n_lig_groups), (nb, n_membrane)):
        assert {0, 1, most} <= seen and any(1 < v < most for v in seen), (name, sorted(seen), most)
    # one hit and one bead are worth more than 100 bounds: a single wrong flag cannot hide inside the bound.  (A pose with no
    # pair inside the 30 A cutoff scores 0.0 and its restraint terms vanish whatever the flags say: the far pose alone.)
    for p, w in enumerate(want):
        assert 999.0 / n_membrane > 100.0 * w["bound"], (name, p)
        if w["pairs"] > 0:
            assert abs(w["score"]) / max(n_rec_groups, n_lig_groups) > 100.0 * w["bound"], (name, p, shifts[p], w["score"], w["bound"])
    assert [p for p, w in enumerate(want) if w["pairs"] == 0] == [len(want) - 1] and shifts[-1] is None
    hip = build_dna(pkg, monkeypatch, shape, rec, lig, method=method)
    got = hip.energy_batch(poses)
    worst = check_within_bound(got, want, (name, method))
    print("%s %s, %d chunks: largest |got - want| / bound = %.2e over %d poses" % (name, method, shape[3], worst, len(poses)))
    assert got[-1] == 0.0
    assert np.array_equal(hip.energy_batch(np.ascontiguousarray(poses[::-1]))[::-1], got)
