"""tests/flag_layouts.py on the CPU, on the oracle alone: the lattice complexes realise the slot layouts and hit counts that
tests/test_gpu_flag_layouts.py holds the pair routes to, and the product's host model lists the same restraint groups and beads
as the oracle's, atom for atom -- the slot order is the order of the restraint CSR followed by the beads (scorer.cpp:
slot_molecule), so equal lists are equal slots.
"""
import numpy as np
import pytest

import flag_layouts as fl


@pytest.fixture(scope="module")
def built(orc, table, tmp_path_factory):
    directory = str(tmp_path_factory.mktemp("flag_layouts"))
    return lambda name: fl.layout(orc, table, directory, name)


def slots_of(model):
    """slot_molecule restated: atom -> slot in the order of the restraint CSR, then the beads; (slots of the CSR, of the beads, words)."""
    slot = {}
    for atom in list(model["restraint_atoms"]) + list(model["membrane"]):
        slot.setdefault(int(atom), len(slot))
    return [slot[int(a)] for a in model["restraint_atoms"]], [slot[int(a)] for a in model["membrane"]], (len(slot) + 31) // 32


def _covers(seen, most, what, name):
    """0, 1 and all of them; a value strictly between 1 and all where there is one."""
    want = {0, 1, most}
    assert want <= seen, (name, what, sorted(want - seen))
    if most > 2:
        assert any(1 < v < most for v in seen), (name, what)


@pytest.mark.parametrize("name", sorted(fl.LAYOUTS))
def test_zero_table_energy_is_the_closed_form_of_the_flags(built, name):
    g = built(name)
    stats = g.stats["zero"]
    assert np.all(stats[:, 0] == 0.0), name                                        # the pair sum of an all-zero table
    assert np.array_equal(g.energy["zero"], fl.closed_form(stats)), name
    # the flags do not depend on the table: the same fractions, pairs and interface atoms under the synthetic one
    assert np.array_equal(stats[:, 2:], g.stats["synth"][:, 2:]), name
    assert np.any(g.stats["synth"][:, 0] != 0.0)
    far = len(g.poses) - 1
    assert g.shifts[far] is None and stats[far, 5] == 0 and g.energy["zero"][far] == 4.7 and g.energy["synth"][far] == 4.7
    if g.sides == "none":
        assert np.all(g.energy["zero"] == 4.7) and np.any(stats[:, 6] > 0)           # atoms do touch; nothing is tracked
    assert len(g.poses) == 17 * (2 * g.rows + 1) + 1 + len(g.wild)


@pytest.mark.parametrize("name", fl.FULL)
def test_every_hit_count_edge_is_realised(built, name):
    g = built(name)
    hr, hl, nb = g.hits()
    print("%s: %d + %d words; receptor hits %s of %d, ligand hits %s of %d, beads %s of %d" % (
        name, slots_of(g.cpu["zero"].model(0))[2], slots_of(g.cpu["zero"].model(1))[2], sorted(set(hr.tolist())), g.n_rec_groups,
        sorted(set(hl.tolist())), g.n_lig_groups, sorted(set(nb.tolist())), g.n_beads))
    # all groups of the ligand -- or, where the ligand is the longer side ((13, 0, 20, .): 13 receptor cells under 20), as many
    # of its named cells as the receptor's cells can lie under at once: those among its first n_rec + beads cells
    lig_most = len([k for k in range(0, g.n_lig, g.every) if k < g.n_rec + g.n_beads]) if g.n_lig_groups else 0
    assert lig_most == g.n_lig_groups or g.sides in ("rec", "lig", "none")
    for seen, most, what in ((hr, g.n_rec_groups, "receptor groups"), (hl, lig_most, "ligand groups"), (nb, g.n_beads, "beads")):
        if most:
            _covers(set(int(v) for v in seen), most, what, name)
            assert max(seen) == most, (name, what)
        else:
            assert not seen.any(), (name, what)
    if g.anm:
        # the shifts go through the amplitudes: the same counts as the rigid lattice's, pose for pose, and the wild poses hit something
        rigid = built("33-25-58-e2")
        n = len(rigid.poses) - 1
        assert g.shifts[:n] == rigid.shifts[:n] and np.array_equal(g.stats["zero"][:n], rigid.stats["zero"][:n])
        amps = g.poses[:, 7:9]
        assert set(np.unique(amps[:n])) == {-2.0, -1.0, 0.0, 1.0, 2.0} and np.all(np.abs(amps[g.wild]) == fl.WILD_AMPLITUDE)
        assert len(g.wild) == 6 and np.all(g.stats["zero"][g.wild, 6] > 0)
        for i in g.wild:
            k = rigid.shifts.index(g.shifts[i])
            assert np.array_equal(g.stats["zero"][i], rigid.stats["zero"][k])


def test_the_bead_ladder_crosses_every_entry_and_exit_of_the_four_trip_loop(built):
    """membrane_beads: lane `sub` of eight enters the unrolled loop while k + 24 < n and leaves the rest to the remainder loop.
    Over the bead counts of the layouts every lane is seen with 0, 1 and 2 unrolled trips -- both entries and both exits are
    crossed between two layouts -- and with an empty and a non-empty remainder loop; the first and the last lane's thresholds
    (n = 25, 57 and n = 32, 64) have a layout on either side, one bead apart."""
    counts = sorted({fl.LAYOUTS[n][1] for n in fl.LAYOUTS if fl.LAYOUTS[n][4] in ("both", "beads")})
    assert set(fl.BEAD_LADDER) <= set(counts) and {1, 7, 9, 25, 33, 64} <= set(counts)
    for sub in range(8):
        trips, rest = set(), set()
        for n in counts:
            k, t = sub, 0
            while k + 24 < n:
                k, t = k + 32, t + 1
            trips.add(t)
            rest.add(len(range(k, n, 8)))
        assert trips == {0, 1, 2} and 0 in rest and max(rest) >= 1, (sub, trips, rest)
    assert {24, 25, 31, 32, 57, 64, 65} <= set(counts)
    for name in ("ladder-%d" % b for b in fl.BEAD_LADDER):
        g = built(name)
        assert set(int(v) for v in g.hits()[2]) >= {0, 1, g.n_beads}


def test_one_hot_layouts_hit_the_named_cells_alone(built):
    """A one-cell ligand over each receptor cell in turn, and a one-cell receptor under each ligand cell: 0 or 1 hit a pose, and a
    hit exactly where the shift puts the single cell on a named cell (or a bead)."""
    g = built("onehot-rec")
    hr, hl, nb = g.hits()
    for i, shift in enumerate(g.shifts[:-1]):
        a, b = shift
        cell = a + 8 * b if 0 <= a < 8 and b >= 0 else -1
        on_named = 0 <= cell < g.n_rec and cell % 2 == 0
        on_bead = g.n_rec <= cell < g.n_rec + g.beads
        on_any = 0 <= cell < g.n_rec + g.beads
        assert (hr[i], nb[i], hl[i]) == (int(on_named), int(on_bead), int(on_any)), g.label(i)
    assert hr.sum() == 17 and nb.sum() == 25
    g = built("onehot-lig")
    hr, hl, nb = g.hits()
    for i, shift in enumerate(g.shifts[:-1]):
        a, b = shift
        cell = -a - 8 * b if -8 < a <= 0 and b <= 0 else -1
        on_any = 0 <= cell < g.n_lig
        assert (hl[i], hr[i], nb[i]) == (int(on_any and cell % 2 == 0), int(on_any), 0), g.label(i)
    assert hl.sum() == 33 and slots_of(g.cpu["zero"].model(1))[2] == 6 and slots_of(g.cpu["zero"].model(0))[2] == 1


def test_slot_layouts_the_lattices_are_for(built):
    """(65, 33, 98, 1) has a group whose five slots straddle a word boundary on either side; the ligand's words and the
    receptor's later words exist; the one-sided layouts leave a side without words."""
    g = built("65-33-98-e1")
    for side in (0, 1):
        model = g.cpu["zero"].model(side)
        group_slots, _, words = slots_of(model)
        offs = model["restraint_offsets"]
        straddling = [k for k in range(len(offs) - 1) if len({s >> 5 for s in group_slots[offs[k]:offs[k + 1]]}) > 1]
        assert straddling and words >= 12, (side, words)
    _, bead_slots, words = slots_of(g.cpu["zero"].model(0))
    assert bead_slots[0] == 325 and words == 12                     # the beads' slots start in the middle of the eleventh word
    for name, want in (("rec-only", (True, False)), ("lig-only", (False, True)), ("beads-only", (True, False)), ("nothing-named", (False, False))):
        g = built(name)
        assert tuple(slots_of(g.cpu["zero"].model(s))[2] > 0 for s in (0, 1)) == want, name


@pytest.mark.parametrize("name", sorted(fl.LAYOUTS))
def test_host_model_lists_the_same_groups_and_beads(built, pkg, name):
    g = built(name)
    for side, path, active in ((0, g.rec_pdb, g.rec_active), (1, g.lig_pdb, g.lig_active)):
        ours, theirs = pkg.model_from_pdb("dfire", path, active=active), g.cpu["zero"].model(side)
        for key in ("coordinates", "dfire_types", "membrane", "restraint_offsets", "restraint_atoms"):
            assert np.array_equal(ours[key], theirs[key]), (name, side, key)
        n_groups = g.n_rec_groups if side == 0 else g.n_lig_groups
        assert len(theirs["restraint_offsets"]) == n_groups + 1 and len(theirs["restraint_atoms"]) == 5 * n_groups
        assert len(theirs["membrane"]) == (g.n_beads if side == 0 else 0)


def _both_models(pkg, orc, path, active):
    """(the host model, the oracle's) of one receptor file, or the two refusals."""
    out = []
    for make in (lambda: pkg.model_from_pdb("dfire", path, active=active),
                 lambda: orc.Scorer("dfire", path, path, rec_active=active, potential=np.zeros(fl.TABLE_LEN)).model(0)):
        try:
            out.append(make())
        except Exception as err:   # a refusal is an answer too: both must refuse
            out.append(err)
    return out


@pytest.mark.parametrize("active,groups,atoms", [
    (["A.ALA.3", "A.ALA.1", "A.ALA.3"], 2, 10),          # an id named twice
    (["A.ALA.1", "M.MMB.15", "M.MMB.20"], 3, 7),         # bead residues named as active restraints
])
def test_inputs_no_fixture_has(built, pkg, orc, active, groups, atoms):
    """Whatever the oracle does with a restraint id named twice, and with a bead that is also a restraint atom (one atom in a
    group and in the bead list: one slot), is the truth, a refusal included; the host model does the same."""
    g = built("13-7-20-e2")
    ours, theirs = _both_models(pkg, orc, g.rec_pdb, active)
    if isinstance(theirs, Exception):
        assert isinstance(ours, Exception), (active, ours)
        return
    assert not isinstance(ours, Exception), ours
    for key in ("membrane", "restraint_offsets", "restraint_atoms"):
        assert np.array_equal(ours[key], theirs[key]), (active, key, ours[key], theirs[key])
    # what the oracle was seen to do (recorded, so that a change of the oracle shows): groups in the order their first atom
    # comes in the file, one group an id however often it is named, a bead's atom listed in its group and among the beads
    assert len(theirs["restraint_offsets"]) - 1 == groups and len(theirs["restraint_atoms"]) == atoms
    assert len(theirs["membrane"]) == 7
    group_slots, bead_slots, words = slots_of(theirs)
    shared = set(group_slots) & set(bead_slots)
    assert len(shared) == (2 if "M.MMB.15" in active else 0) and words == 1
