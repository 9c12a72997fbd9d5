"""CPU side of the energy decomposition (include/lightdock_hip.h "Energy decomposition"): the residue maps of the host
model builder (ld_model_num_residues / ld_model_residue_id / ld_model_residue_of_atom), the constants the Python binding
mirrors from the header, the layout of ld_energy_terms / ld_group_energies in the binding and in the Rust crate, and
decompose.py's scaling to score units and its two list formats on made-up arrays.  No GPU."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import test_rust_binding as rb
from test_analysis_cpu import tool_module

HEADER = os.path.join(ROOT, "include", "lightdock_hip.h")


def tool():
    return tool_module("decompose")


def file_residue_ids(path):
    """Distinct "<chain>.<resname>.<serial><icode>" of a PDB file's ATOM / HETATM records, in first-appearance order."""
    ids = []
    for line in open(path):
        if line.startswith(("ATOM  ", "HETATM")):
            rid = "%s.%s.%d%s" % (line[21].strip(), line[17:20].strip(), int(line[22:26]), line[26].strip())
            if rid not in ids:
                ids.append(rid)
    return ids


@pytest.mark.parametrize("name,method,pdb", [("1ppe", "dfire", "lightdock_1ppe_e.pdb"), ("1ppe", "dfire", "lightdock_1ppe_i.pdb"),
                                             ("1azp", "dna", "lightdock_protein.pdb"), ("1azp", "dna", "lightdock_dna.pdb"),
                                             ("ab_icode", "dfire", "lightdock_receptor.pdb"), ("ab_icode", "dfire", "lightdock_ligand.pdb")])
def test_residue_maps_of_the_model_builder(pkg, name, method, pdb):
    path = os.path.join(GOLDEN, name, pdb)
    m = pkg.model_from_pdb(method, path)
    residues, of_atom = m["residues"], m["residue_of_atom"]
    n = m["coordinates"].shape[0]
    want = file_residue_ids(path)
    assert len(set(residues)) == len(residues) and sorted(residues) == sorted(want)     # one per residue id
    assert of_atom.shape == (n,) and of_atom.dtype == np.uint32                          # every atom
    assert of_atom[0] == 0 and np.all(np.diff(of_atom.astype(np.int64)) >= 0)            # ascending
    assert np.array_equal(np.unique(of_atom), np.arange(len(residues)))                  # every residue has atoms
    if name == "ab_icode" and pdb == "lightdock_receptor.pdb":
        assert "H.ASP.52A" in residues and "H.LEU.82C" in residues       # insertion codes make residues of their own
        assert np.count_nonzero(of_atom == residues.index("H.ASP.52A")) == 8
    # the restraint atoms of a residue are exactly the atoms the map gives it
    rid = residues[len(residues) // 2]
    r = pkg.model_from_pdb(method, path, active=[rid])
    assert np.array_equal(r["restraint_atoms"], np.flatnonzero(of_atom == residues.index(rid)))


def test_residue_entry_points_refuse_by_status(pkg):
    import ctypes as C
    lib = pkg.load_library()
    buf = C.create_string_buffer(64)
    assert lib.ld_model_num_residues(None) == 0
    assert lib.ld_model_residue_id(None, 0, buf, 64) == -1 and lib.ld_model_residue_of_atom(None, None) == -1
    h = C.c_void_p(lib.ld_model_from_pdb(0, os.fsencode(os.path.join(GOLDEN, "1ppe", "lightdock_1ppe_i.pdb")), None, 0, None, 0, None, 0, 0))
    assert h
    n = lib.ld_model_num_residues(h)
    assert n > 0 and lib.ld_model_residue_id(h, n, buf, 64) == -1          # index out of range
    assert lib.ld_model_residue_id(h, 0, buf, 3) == -1                     # buffer too short
    assert lib.ld_model_residue_id(h, 0, buf, 64) == 0 and buf.value.decode().count(".") == 2
    lib.ld_model_destroy(h)


def test_binding_mirrors_the_header(pkg):
    text = open(HEADER).read()
    assert int(re.search(r"#define LD_GROUP_NONE \((0x[0-9a-f]+)u\)", text).group(1), 16) == pkg.GROUP_NONE
    # the chunk size is the kernels' own; the GPU suite's chunk-edge shape follows it
    import test_gpu_decompose as tg
    kernels = open(os.path.join(ROOT, "lightdock-rust_amd", "csrc", "kernels", "decompose.hpp")).read()
    assert int(re.search(r"constexpr int kDecomposeChunk = (\d+);", kernels).group(1)) == tg.PARTNER_CHUNK
    assert "PARTNER_CHUNK" not in text
    hs, hf = rb.parse_header(text)
    c_to_np = {"f64": np.float64, "u32": np.uint32}
    fields = hs["ld_energy_terms"]
    assert [n for n, _ in fields] == list(pkg.ENERGY_TERMS.names)
    for name, t in fields:
        sub = pkg.ENERGY_TERMS[name]
        if name == "pair":
            assert t == "*mut f64" and sub.shape == (2,) and sub.base == np.float64    # `double pair[2]` as the parser prints an array
        else:
            assert sub == np.dtype(c_to_np[t])
    assert pkg.ENERGY_TERMS.itemsize == 7 * 8 + 4 * 4 and pkg.ENERGY_TERMS.isalignedstruct is False
    assert [pkg.ENERGY_TERMS.fields[n][1] for n in pkg.ENERGY_TERMS.names] == [0, 16, 24, 32, 40, 48, 56, 60, 64, 68]
    want = [("group_of_atom", "*const u32"), ("n_groups", "usize"), ("sums", "*mut f64"), ("pairs", "*mut u32"), ("interface_atoms", "*mut u32")]
    assert hs["ld_group_energies"] == want
    assert [n for n, _ in pkg._GroupEnergies._fields_] == [n for n, _ in want]
    assert hf["ld_scorer_decompose"][1][4][0] == "*mut ld_energy_terms" and hf["ld_scorer_decompose"][1][5][0] == "*const ld_group_energies"


def test_rust_crate_declares_the_decomposition_structs():
    """The two structs' layouts in bindings/rust/lightdock-hip/src/lib.rs against the header, with test_rust_binding's parsers;
    the entry points themselves are compared by test_rust_binding.py::test_binding_crate_matches_the_header."""
    hs, hf = rb.parse_header(open(HEADER).read())
    rs, rf = rb.parse_rust(open(rb.LIB_RS).read())
    for name in ("ld_scorer_decompose", "ld_scorer_decompose_info", "ld_model_from_pdb", "ld_model_destroy", "ld_model_num_residues",
                 "ld_model_residue_id", "ld_model_residue_of_atom"):
        assert name in rf and name in hf, name
    for c_name in ("ld_energy_terms", "ld_group_energies"):
        assert c_name in rs, "%s: #[repr(C)] struct missing" % c_name
        want, got = hs[c_name], rs[c_name]
        assert [n for n, _ in want] == [n for n, _ in got]
        for (n, tw), (_, tg) in zip(want, got):
            assert tg == ("[f64; 2]" if n == "pair" else tw), (c_name, n, tg, tw)


def test_score_units_and_penalty():
    t = tool()
    sums = np.array([[[2.0, 0.0], [-1.5, 0.0]], [[0.0, 0.0], [100.0, 0.0]]])
    u = t.score_units(sums, True)
    assert u.shape == (2, 2, 1) and np.array_equal(u[..., 0], sums[..., 0] * 0.0157 * -1.0)
    # a pose's residues add up to its score less the constant: (sum * 0.0157 - 4.7) * -1
    assert abs(u[0].sum() - ((sums[0, :, 0].sum() * 0.0157 - 4.7) * -1.0 - 4.7)) < 1e-15
    sums = np.array([[[0.25, -3.0], [-0.5, 1.0]]])
    u = t.score_units(sums, False)
    assert u.shape == (1, 2, 3)
    assert np.array_equal(u[0, :, 0], [-0.25 * 83.0, 0.5 * 83.0]) and np.array_equal(u[0, :, 1], [3.0, -1.0])
    assert np.array_equal(u[0, :, 2], u[0, :, 0] + u[0, :, 1])
    assert abs(u[0, :, 2].sum() - (-(sums[0, :, 0].sum() * 332.0 / 4.0 + sums[0, :, 1].sum()))) < 1e-12
    assert np.isnan(t.score_units(np.array([[np.nan, 1.0]]), False)[0, 2])
    assert np.array_equal(t.penalty([0.0, 0.5, 1.0 / 3.0]), [0.0, 499.5, 999.0 * (1.0 / 3.0)])


@pytest.mark.parametrize("dfire", [True, False])
def test_list_formats_round_trip(pkg, dfire):
    t = tool()
    entries = [(3, 17, None, {"scoring": 12.345678}), (0, 4, None, {"scoring": -1.0})]
    terms = np.zeros(2, dtype=pkg.ENERGY_TERMS)
    terms["pair"] = [[-1234.5678901234567, 0.0 if dfire else 7.25], [1.0 / 3.0, 0.0 if dfire else -2.0 / 7.0]]
    terms["score"] = [24.082716049382716, -4.7]
    terms["energy"] = [48.165432098765432, np.nan]
    terms["rec_restraints"], terms["lig_restraints"], terms["membrane"] = [1.0, 0.0], [0.0, 0.5], [0.0, 0.25]
    terms["pairs"] = [114321, 0]
    head, rows = t.parse_list(t.terms_text(entries, terms, dfire))
    assert head == (["Swarm", "Glowworm", "Scoring", "Energy", "Score"] + (["Pair"] if dfire else ["Elec", "VdW"]) +
                    ["Rec", "Lig", "Beads", "Penalty", "Pairs"])
    assert len(rows) == 2 and all(len(r) == len(head) for r in rows)
    col = {h: [r[k] for r in rows] for k, h in enumerate(head)}
    assert [int(v) for v in col["Swarm"]] == [3, 0] and [int(v) for v in col["Glowworm"]] == [17, 4]
    assert [float(v) for v in col["Scoring"]] == [12.34568, -1.0]
    assert float(col["Energy"][0]) == terms["energy"][0] and np.isnan(float(col["Energy"][1]))       # 17 digits: the same doubles
    assert [float(v) for v in col["Score"]] == list(terms["score"])
    assert [float(v) for v in col["Pair" if dfire else "Elec"]] == list(terms["pair"][:, 0])
    if not dfire:
        assert [float(v) for v in col["VdW"]] == list(terms["pair"][:, 1])
    assert [float(v) for v in col["Beads"]] == [0.0, 0.25] and [float(v) for v in col["Penalty"]] == [0.0, 249.75]
    assert [int(v) for v in col["Pairs"]] == [114321, 0]

    ids = ["A.SER.467", "H.ASP.52A", "A.GLY.1"]
    rec = {"sums": np.array([[[1.5, -0.5], [0.0, 0.0], [-2.0, 0.125]], [[0.0, 0.0], [0.1, 0.2], [0.0, 0.0]]]),
           "pairs": np.array([[10, 0, 3], [0, 1, 0]], dtype=np.uint32), "interface": np.array([[2, 0, 0], [0, 1, 0]], dtype=np.uint32)}
    lig = {"sums": np.array([[[0.75, 0.0]], [[0.0, 0.0]]]), "pairs": np.array([[13], [0]], dtype=np.uint32),
           "interface": np.array([[1], [0]], dtype=np.uint32)}
    head, rows = t.parse_list(t.residues_text(entries, (("R", ids, rec), ("L", ["B.DT.13"], lig)), dfire))
    assert head == ["Swarm", "Glowworm", "Side", "Residue"] + (["Energy"] if dfire else ["Elec", "VdW", "Energy"]) + ["Pairs", "Interface"]
    # only residues with a pair inside the cutoff, candidates in order, receptor before ligand
    assert [(int(r[0]), int(r[1]), r[2], r[3]) for r in rows] == [(3, 17, "R", "A.SER.467"), (3, 17, "R", "A.GLY.1"), (3, 17, "L", "B.DT.13"),
                                                                  (0, 4, "R", "H.ASP.52A")]
    e = head.index("Energy")
    want = t.score_units(rec["sums"], dfire)
    assert float(rows[0][e]) == want[0, 0, -1] and float(rows[1][e]) == want[0, 2, -1] and float(rows[3][e]) == want[1, 1, -1]
    assert [int(r[-2]) for r in rows] == [10, 3, 13, 1] and [int(r[-1]) for r in rows] == [2, 0, 1, 1]
