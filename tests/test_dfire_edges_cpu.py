"""tests/dfire_edges.py on the CPU: every knife edge of every geometry is realised by the oracle alone, with nothing left out,
and the replay of the block-major f32 arithmetic stays inside the bound the LUT is built for.

The replay's figure is |E_f32 - (seed - 64 d2_f64)| / eps for the target pair of every pose.  A LUT is correct while that
stays below 1 (scorer.cpp, dfire_bm_error_bound, derives eps as twice its bound on the error: it targets 0.5).  Two eps:
  eps          pkg.dfire_bm_lut(ubound, lig_extent): the frame's bound with every receptor subtile inside what the derivation
               assumes (|r - c| < 32 A a coordinate, |l - c| < 45 A).  It was the scorer's bound for EVERY complex until the widest
               subtile box entered it; the ratio against it is asserted for G1-G5 and W1, which satisfy the assumptions, and PRINTED,
               not asserted, for the wide subtiles W2-W4: the measurement of what an unenforced assumption cost (W4: above 1).
  eps_scorer   the bound bm_accepts derives, the receptor's widest subtile box in it (pkg.dfire_route_frames with the types):
               asserted below 1 for every geometry.  Equal to eps, bit for bit, wherever the assumptions hold.
The replay also reads the LUT at floor(E) and holds its answer against the oracle's: a cell that is not flagged must name the
oracle's bin (or a miss where the oracle counts no pair).  W5 (H = 400 A) is the shape the old bound got wrong: the replay
decides hundreds of its rungs wrongly with the LUT of eps, and bm_accepts now declines it (eps_scorer >= 8 cells).

Sensitivity, on the CPU.  (a) The same f32 cells through the LUT the library builds for a frame an eighth of the size (eps some
six times smaller) decide NO rung wrongly, and no finer ladder could make them: every bin step sits at the middle of a LUT cell,
so a pair is binned wrongly only if its f32 distance is off by more than 1/2 cell + the LUT's eps, and the f32 error of these
shapes (0.23 cells at G5, printed) stays below half a cell -- dfire_bm_error_bound is some twenty times what compact shapes
show.  (b) What the ladder does resolve: a route that read the bin off its f32 distance alone, with no exact path, decides dozens of
rungs wrongly in every geometry, most of them further than an ulp from the edge.
"""
import numpy as np
import pytest

import dfire_edges
from dfire_edges import FLAGGED, G_UBOUNDS, GEOMETRIES, N_RUNGS, W_HALF

ALL = GEOMETRIES + ("G3anm",)


@pytest.fixture(scope="module")
def built(pkg, orc, table, tmp_path_factory):
    directory = str(tmp_path_factory.mktemp("dfire_edges"))
    return lambda name: dfire_edges.geometry(pkg, orc, table, directory, name)


@pytest.mark.parametrize("name", ALL)
def test_every_edge_is_realised_by_the_oracle(built, pkg, name):
    g = built(name)
    for batch in g.batches:
        assert g.poses[batch].shape == (3 * 22 * N_RUNGS, 13 if g.anm else 7)
        assert len(g.brackets[batch]) == 3 * 22                       # rho0, rho1 found for every edge: the share left out is 0
        rho0, rho1 = g.brackets[batch].T
        assert np.all(np.nextafter(rho0, np.inf) == rho1)
        assert np.all(np.abs(rho0 - np.tile(g.nominal, 3)) < dfire_edges.BRACKET)
    dfire_edges.check_edges(g)
    bm = g.frames["bm"]
    print("%s: h %.3f A, block-major frame %g units, eps %.4f cells, lig_extent %g, target subtile half extent %.2f A; packed frame %g, eps %.2e"
          % (name, g.h, bm["ubound"], bm["eps"], bm["lig_extent"], g.sub_half, g.frames["packed"]["ubound"], g.frames["packed"]["eps"]))
    assert bm["takes"] and g.frames["packed"]["takes"]
    assert bm["lig_extent"] == np.abs(g.lig_xyz).max() == 52.137
    if name in W_HALF:
        assert len(g.rec_xyz) == 8 and g.sub_half >= 0.9 * W_HALF[name]
    else:
        assert g.sub_half <= 16.0
        assert bm["ubound"] == G_UBOUNDS.get(name[:2], bm["ubound"])


def test_the_largest_frame_and_one_step_further(built, pkg):
    """G5 is the last frame the block-major route takes; 1/8 A more (G6) doubles the frame and the route declines."""
    g5, g6 = built("G5"), built("G6")
    assert g5.frames["bm"]["takes"] and g5.frames["bm"]["eps"] < 8.0
    assert not g6.frames["bm"]["takes"] and g6.frames["bm"]["ubound"] == 2.0 * g5.frames["bm"]["ubound"] and g6.h == g5.h + 0.125
    assert g6.frames["packed"]["takes"]
    dfire_edges.check_edges(g6)


@pytest.mark.parametrize("name", GEOMETRIES)
def test_replay_of_the_block_major_arithmetic(built, pkg, name):
    g = built(name)
    r = dfire_edges.replay(pkg, g)
    worst = int(np.argmax(r["ratio"]))
    wrong = dfire_edges.decisions_of(g, r["code"])
    flagged = r["code"] == FLAGGED
    print("%s: max |E_f32 - E| %.4f cells = %.3f eps (eps %.4f) at %s; operands |r-c| %.1f |l-c| %.1f |l-c|^2 %.3g; %d of %d poses flagged, %d decided wrongly"
          % (name, r["err"].max(), r["ratio"].max(), r["eps"], g.label(worst), r["operands"]["r_minus_c"], r["operands"]["l_minus_c"],
             r["operands"]["l2"], flagged.sum(), len(flagged), wrong.sum()))
    # the premise of the exact-path checks on the GPU: rho0 and rho1 of every step and of the cutoff are flagged
    k = len(dfire_edges.RUNG_KS)
    for rot in range(3):
        for e in range(22):
            if e != 20:
                assert flagged[g.index(rot, e, k)] and flagged[g.index(rot, e, k + 1)], g.label(g.index(rot, e, k))
    assert r["err"].max() / r["eps_scorer"] < 1.0, g.label(worst)
    assert not wrong.any(), [g.label(i) for i in np.flatnonzero(wrong)[:4]]
    if name in ("W2", "W3", "W4"):
        assert r["eps_scorer"] > r["eps"]
        return                       # the ratio against eps: measured, not asserted (module docstring)
    assert r["eps_scorer"] == r["eps"]
    assert r["ratio"].max() < 1.0, g.label(worst)


def test_a_subtile_wider_than_the_bound_covers_is_declined(built, pkg):
    """W5, two groups of four atoms 400 A either side of the subtile's centre: with the LUT of the bound that assumed compact
    subtiles the replay decides rungs wrongly; the bound with the subtile in it reaches 8 cells and the route declines."""
    g = built("W5")
    dfire_edges.check_edges(g)
    assert g.sub_half >= 0.9 * W_HALF["W5"]
    assert g.frames_compact["bm"]["takes"] and not g.frames["bm"]["takes"] and g.frames["bm"]["eps"] >= 8.0
    assert g.frames["packed"]["takes"]
    r = dfire_edges.replay(pkg, g)
    wrong = dfire_edges.decisions_of(g, r["code"])
    print("W5: max |E_f32 - E| %.3f cells = %.2f eps (eps %.3f, with the subtile %.1f); %d of %d rungs decided wrongly by the LUT of eps"
          % (r["err"].max(), r["ratio"].max(), r["eps"], r["eps_scorer"], wrong.sum(), len(wrong)))
    assert r["ratio"].max() > 1.0 and wrong.sum() > 100


def test_what_a_wrong_lut_would_have_to_be_to_fail_the_ladder(built, pkg, orc):
    """Sensitivity (module docstring): (a) G4 and G5 through the LUT of a frame an eighth of their size; (b) every geometry with
    the bin read off the f32 distance alone."""
    for name in ("G4", "G5"):
        g = built(name)
        r = dfire_edges.replay(pkg, g)
        f = g.frames["bm"]
        codes, eps_small = pkg.dfire_bm_lut(f["ubound"] / 8.0, f["lig_extent"])
        wrong = dfire_edges.decisions_of(g, codes[np.minimum(r["cell"], len(codes) - 1)])
        print("%s: eps %.3f -> %.3f cells: %d rungs decided wrongly; the f32 error reaches %.3f cells, the narrow LUT flags within %.3f"
              % (name, r["eps"], eps_small, wrong.sum(), r["err"].max(), 0.5 + eps_small))
        assert r["err"].max() < 0.5 and not wrong.any()
    for name in GEOMETRIES:
        g = built(name)
        r = dfire_edges.replay(pkg, g)
        d2 = (dfire_edges.SEED_CELL - r["E"].astype(np.float64)) / 64.0
        code = np.array([8 * orc.dfire_bin(v) if v <= 225.0 else dfire_edges.MISS for v in d2])
        wrong = dfire_edges.decisions_of(g, code) & ~g.special["rigid"]
        k = len(dfire_edges.RUNG_KS)
        rung = np.arange(len(wrong)) % N_RUNGS
        print("%s: the f32 distance alone decides %d rungs wrongly, %d of them further than an ulp from the edge" % (
            name, wrong.sum(), (wrong & (rung != k) & (rung != k + 1)).sum()))
        assert wrong.sum() >= 20 and (wrong & (rung != k) & (rung != k + 1)).sum() >= 20, name
