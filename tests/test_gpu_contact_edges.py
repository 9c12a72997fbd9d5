"""Residue contacts on the MI355X ON their threshold at every pruning level: ld_complex_contacts (complex_contacts,
kernels/cluster.hip) and ld_complex_pair_contacts (complex_pair_sets, kernels/fcc.hip) against the all-pairs int64 oracle of
tests/contact_edges.py at every case built there.  Every comparison is exact equality of boolean or integer arrays; no case is
left out.  tests/test_contact_edges_cpu.py proves on the CPU what each case covers: the box level that decides, the place in
the walk, the deciding atom, the scan chunk of the pair bitmap, the skip of complex_contacts."""
import ctypes

import numpy as np
import pytest

import contact_edges as ce

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def complexes(pkg, tmp_path_factory):
    """shape name -> Complex, each built once."""
    pkg.init(0)
    directory = str(tmp_path_factory.mktemp("contact_edges"))
    made = {}

    def get(name):
        if name not in made:
            sh = ce.shape(name)
            made[name] = ce.make_complex(pkg, sh, directory)
            cx = made[name]
            assert (cx.num_residues(0), cx.num_residues(1), cx.pose_len) == (sh.n_rec_res, sh.n_lig_res, sh.pose_len)
            assert np.array_equal(cx.residue_of_atom(0), sh.rec_of) and np.array_equal(cx.residue_of_atom(1), sh.lig_of)
        return made[name]

    return get


def first_difference(got, want, case):
    i = int(np.flatnonzero((got != want).any(axis=1))[0])
    return case.name, i, case.poses[i], np.flatnonzero(got[i]), np.flatnonzero(want[i])


def check_case(cx, case):
    """Both calls on every pose of the case against the oracle; the residues the keys name are the contact bits."""
    sh = ce.shape(case.shape)
    poses, cutoff = ce.rows(sh, case.poses), case.C / 1000.0
    want_rec, want_lig, want_offsets, want_keys = ce.expected_words(case.name)
    got = cx.contacts(poses, cutoff)
    for side, want in (("rec", want_rec), ("lig", want_lig)):
        assert got[side].shape == want.shape and got[side].dtype == bool
        assert np.array_equal(got[side], want), ("contacts", side) + first_difference(got[side], want, case)
    offsets, keys = cx.pair_contacts(poses, cutoff)
    assert np.array_equal(offsets, want_offsets), ("pair counts", case.name, np.flatnonzero(np.diff(offsets.astype(np.int64)) != np.diff(want_offsets))[:8])
    assert np.array_equal(keys, want_keys), ("pair keys", case.name)
    for i in range(len(poses)):
        assert np.all(np.diff(keys[offsets[i]:offsets[i + 1]].astype(np.int64)) > 0), (case.name, i)
    rec, lig = ce.projection(sh, offsets, keys)
    assert np.array_equal(rec, got["rec"]) and np.array_equal(lig, got["lig"]), case.name
    return got, offsets, keys


@pytest.mark.parametrize("name", ce.CASE_NAMES)
def test_every_case_word_for_word(complexes, name):
    """The level that decides, the places in the walk, the deciding atom and the scan chunks on the 520 x 517 complex, rigid,
    flexing and with boxes beyond LDS; d^2 == C^2 and the sum above on one, two and three axes in every order and sign at 5.0, 30.0
    and 0.001 A; differences a 32-bit sum of squares would wrap; the six residues of the skip."""
    case = ce.case_named(name)
    got, offsets, _ = check_case(complexes(case.shape), case)
    kinds = [p.kind for p in case.poses]
    print("%s: %d poses, %d in, %d out; %d poses with a contact, %d keys" % (name, len(kinds), kinds.count("in"), kinds.count("out"),
                                                                         int(got["rec"].any(axis=1).sum()), int(offsets[-1])))


@pytest.mark.parametrize("name", ["edges-base-C5000", "edges-flex-C5000", "edges-big-C5000", "motif"])
def test_pieces_and_reused_slots_give_the_same_words(complexes, name):
    """All poses of a case in one call, the same poses in two pieces, and the list eight times over -- more poses than workspace
    slots, so that a workgroup's slot, its boxes and its pair bitmap serve other poses in turn -- give the same words."""
    case = ce.case_named(name)
    sh, cx = ce.shape(case.shape), complexes(case.shape)
    poses, cutoff = ce.rows(sh, case.poses), case.C / 1000.0
    n = len(poses)
    check_case(cx, case)
    _, _, want_offsets, want_keys = ce.expected_words(case.name)
    whole = cx.contacts(poses, cutoff, packed=True)
    cut = n // 2 + 1
    pieces = [cx.contacts(poses[a:b], cutoff, packed=True) for a, b in ((0, cut), (cut, n))]
    for side in ("rec", "lig"):
        assert np.array_equal(np.concatenate([p[side] for p in pieces]), whole[side]), (name, side)
    parts = [cx.pair_contacts(poses[a:b], cutoff) for a, b in ((0, cut), (cut, n))]
    assert np.array_equal(np.concatenate([k for _, k in parts]), want_keys)
    assert np.array_equal(np.concatenate([parts[0][0], parts[1][0][1:] + parts[0][0][-1]]), want_offsets)
    times = 8 if n > 128 else 260
    assert times * n > 1024                                         # kContactSlots, kPairSlots
    order = np.random.default_rng(3).permutation(times * n) % n     # a slot's poses in turn are not each other's copies
    many = cx.contacts(poses[order], cutoff, packed=True)
    for side in ("rec", "lig"):
        assert np.array_equal(many[side], whole[side][order]), (name, side)
    offsets, keys = cx.pair_contacts(poses[order], cutoff)
    sets = [want_keys[want_offsets[i]:want_offsets[i + 1]] for i in range(n)]
    assert np.array_equal(np.diff(offsets.astype(np.int64)), np.diff(want_offsets)[order])
    assert np.array_equal(keys, np.concatenate([sets[i] for i in order]))


@pytest.mark.parametrize("name", ["edges-base-C5000", "edges-big-C5000", "motif"])
def test_the_count_only_call_agrees_with_the_filling_call(pkg, complexes, name):
    case = ce.case_named(name)
    sh, cx, lib = ce.shape(case.shape), complexes(case.shape), pkg.load_library()
    poses = np.ascontiguousarray(ce.rows(sh, case.poses))
    n = len(poses)
    _, _, want_offsets, want_keys = ce.expected_words(case.name)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    counted, total = np.full(n + 1, 0xA5A5A5A5, dtype=np.uint32), ctypes.c_size_t(12345)
    assert lib.ld_complex_pair_contacts(cx._h, n, ptr(poses), poses.shape[1], ctypes.c_double(case.C / 1000.0), ptr(counted), None, 0,
                                        ctypes.byref(total)) == 0
    assert total.value == len(want_keys) and np.array_equal(counted, want_offsets)
    filled, keys = np.zeros(n + 1, dtype=np.uint32), np.full(total.value + 1, 0xA5A5A5A5, dtype=np.uint32)
    assert lib.ld_complex_pair_contacts(cx._h, n, ptr(poses), poses.shape[1], ctypes.c_double(case.C / 1000.0), ptr(filled), ptr(keys),
                                        total.value, ctypes.byref(total)) == 0
    assert np.array_equal(filled, counted) and np.array_equal(keys[:-1], want_keys) and keys[-1] == 0xA5A5A5A5


def test_boxes_in_lds_and_in_global_memory_agree(complexes):
    """The poses base and big share (the long ligand's first 517 residues are base's ligand, the rest never comes near): the
    same receptor bits, the same ligand bits, the same pairs."""
    base, big = ce.edge_case("base"), ce.edge_case("big")
    sb, sg = ce.shape("base"), ce.shape("big")
    assert sb.boxes_in_lds and not sg.boxes_in_lds
    shared = [i for i, (p, q) in enumerate(zip(base.poses, big.poses)) if p == q]
    assert len(shared) >= 120
    poses = ce.rows(sb, [base.poses[i] for i in shared])
    lds, glob = complexes("base").contacts(poses, 5.0), complexes("big").contacts(poses, 5.0)
    assert lds["rec"].any() and np.array_equal(lds["rec"], glob["rec"])
    assert np.array_equal(lds["lig"], glob["lig"][:, :sb.n_lig_res]) and not glob["lig"][:, sb.n_lig_res:].any()
    (ob, kb), (og, kg) = complexes("base").pair_contacts(poses, 5.0), complexes("big").pair_contacts(poses, 5.0)
    assert np.array_equal(ob, og)
    kb, kg = kb.astype(np.int64), kg.astype(np.int64)
    assert np.array_equal(kb // sb.n_lig_res, kg // sg.n_lig_res) and np.array_equal(kb % sb.n_lig_res, kg % sg.n_lig_res)
