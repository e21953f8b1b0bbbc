"""CPU: the float64 restatement of tests/score_refs.py against numbers worked out by hand (two-atom systems at every breakpoint of the
five terms), the typing rules of fabind_amd.scoring against hand molecules and against the restatement's atom-by-atom typing, the
residue table against the entries DESIGN.md section 22 lists, and the wiring of the entry point."""
import os
import re

import numpy as np
import pytest
import torch

import score_refs as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, D, A = SR.HYDROPHOBIC, SR.DONOR, SR.ACCEPTOR
W = SR.WEIGHTS


def _two(r, ti, tj, **kw):
    """A ligand atom of word ti at the origin and a protein atom of word tj at distance r on the x axis."""
    return SR.score(np.zeros((1, 3), np.float32), [ti], np.array([[r, 0, 0]], np.float32), [6], [tj], **kw)


def _at(d, ti, tj, **kw):
    """The same with the distance chosen for a surface distance d (r rounded to float32: d is recomputed from it)."""
    r = np.float32(d + SR.RADII[ti & 15] + SR.RADII[tj & 15])
    return _two(r, ti, tj, **kw), (np.float64(r) - SR.RADII[ti & 15]) - SR.RADII[tj & 15]


# ------------------------------------------------------------------------------------------------ the energy, by hand
def test_two_carbons_in_contact_by_hand():
    # C (1.9) and C (1.9) at r = 3.8: d = 0 exactly -> gauss1 = 1, gauss2 = exp(-2.25), repulsion 0, hydrophobic 1 (both carbons), no hbond
    out = _two(3.8, SR.C_ | H, SR.C_ | H)
    d = (np.float64(np.float32(3.8)) - 1.9) - 1.9
    assert abs(d) < 1e-7 and out["n_pairs"] == 1 and out["flags"] == 0
    want = [np.exp(-(d / 0.5) ** 2), np.exp(-((d - 3) / 2) ** 2), d * d if d < 0 else 0.0, 1.0, 0.0]
    np.testing.assert_allclose(out["terms"], want, rtol=1e-15, atol=1e-300)
    assert abs(out["terms"][0] - 1.0) < 1e-12 and abs(out["terms"][1] - np.exp(-2.25)) < 1e-7
    inter = W[0] * want[0] + W[1] * want[1] + W[2] * want[2] + W[3] * want[3] + W[4] * want[4]
    assert abs(out["inter"] - inter) < 1e-15 and abs(out["inter"] - (-0.035579 - 0.005156 * np.exp(-2.25) - 0.035069)) < 1e-8
    assert out["total"] == out["inter"] and out["per_atom"].tolist() == [out["inter"]]
    assert abs(out["abs_inter"] - (0.035579 + 0.005156 * np.exp(-2.25) + 0.035069)) < 1e-8


@pytest.mark.parametrize("d, want", [(-0.8, 1.0), (-0.7001, 1.0), (-0.6999, 0.6999 / 0.7), (-0.35, 0.5), (-1e-4, 1e-4 / 0.7), (1e-4, 0.0), (0.5, 0.0)])
def test_hbond_breakpoints(d, want):
    out, dd = _at(d, SR.N_ | D, SR.O_ | A)
    assert abs(dd - d) < 1e-6
    exact = 1.0 if dd < -0.7 else -dd / 0.7 if dd < 0 else 0.0
    assert out["terms"][4] == exact and abs(exact - want) < 2e-6
    assert out["terms"][3] == 0.0                                        # neither atom is hydrophobic
    assert out["terms"][2] == (dd * dd if dd < 0 else 0.0)


@pytest.mark.parametrize("d, want", [(-0.2, 1.0), (0.4999, 1.0), (0.5001, 0.9999), (1.0, 0.5), (1.4999, 1e-4), (1.5001, 0.0), (3.0, 0.0)])
def test_hydrophobic_breakpoints(d, want):
    out, dd = _at(d, SR.C_ | H, SR.CL_ | H)
    exact = 1.0 if dd < 0.5 else 1.5 - dd if dd < 1.5 else 0.0
    assert out["terms"][3] == exact and abs(exact - want) < 2e-6 and out["terms"][4] == 0.0


@pytest.mark.parametrize("d", [-0.5, -1e-4, 1e-4, 0.5])
def test_repulsion_breakpoint_and_gaussians(d):
    out, dd = _at(d, SR.S_, SR.P_)
    assert out["terms"][2] == (dd * dd if dd < 0 else 0.0)
    assert (out["terms"][2] > 0) == (d < 0)
    assert out["terms"][0] == np.exp(-((dd / 0.5) * (dd / 0.5))) and out["terms"][1] == np.exp(-(((dd - 3.0) / 2.0) * ((dd - 3.0) / 2.0)))
    assert out["terms"][3] == 0.0 and out["terms"][4] == 0.0


def test_the_exact_breakpoint_values():
    # the piecewise definitions AT their breakpoints, on d given directly: -0.7 -> -d / 0.7 = 1 (both branches agree), 0 -> 0,
    # 0.5 -> 1.5 - d = 1, 1.5 -> 0
    t = SR.pair_terms(np.array([-0.7, 0.0, 0.5, 1.5]), np.full(4, SR.C_ | H | D), np.full(4, SR.C_ | H | A))
    assert t[:, 4].tolist() == [1.0, 0.0, 0.0, 0.0] and t[:, 3].tolist() == [1.0, 1.0, 1.0, 0.0] and t[:, 2].tolist() == [0.7 * 0.7, 0.0, 0.0, 0.0]


def test_cutoff_is_strict_and_compared_on_r_squared():
    far = _two(8.0, SR.C_ | H, SR.C_ | H)                                # r = 8 exactly: excluded
    assert far["n_pairs"] == 0 and far["terms"].tolist() == [0.0] * 5 and far["inter"] == 0.0 and far["cut_margin"] == 0.0
    near = _two(np.nextafter(np.float32(8.0), np.float32(0.0)), SR.C_ | H, SR.C_ | H)
    assert near["n_pairs"] == 1 and near["terms"][1] > 0.0
    assert _two(7.5, SR.C_, SR.C_, cutoff=7.5)["n_pairs"] == 0 and _two(7.5, SR.C_, SR.C_, cutoff=7.6)["n_pairs"] == 1


def test_role_gating():
    d = -0.3
    assert _at(d, SR.N_ | D, SR.N_ | D)[0]["terms"][4] == 0.0           # a donor with a donor
    assert _at(d, SR.O_ | A, SR.O_ | A)[0]["terms"][4] == 0.0           # an acceptor with an acceptor
    assert _at(d, SR.O_ | A, SR.N_ | D)[0]["terms"][4] > 0.0            # either direction
    assert _at(d, SR.N_ | D, SR.O_ | A)[0]["terms"][4] > 0.0
    assert _at(d, SR.O_ | D | A, SR.O_ | D | A)[0]["terms"][4] > 0.0
    assert _at(d, SR.C_ | H, SR.C_)[0]["terms"][3] == 0.0               # one hydrophobic atom alone
    assert _at(d, SR.C_, SR.C_ | H)[0]["terms"][3] == 0.0
    assert _at(d, SR.C_ | H, SR.C_ | H)[0]["terms"][3] == 1.0
    assert _at(d, SR.METAL_ | D, SR.O_ | A)[0]["terms"][4] > 0.0        # a metal is a donor


def test_torsion_scaling_weights_and_hydrogens_dropped():
    base = _two(4.0, SR.C_ | H, SR.C_ | H)
    for nt in (0, 1, 7):
        out = _two(4.0, SR.C_ | H, SR.C_ | H, n_torsions=nt)
        assert out["inter"] == base["inter"] and out["total"] == base["inter"] / (1.0 + 0.0585 * nt)
    assert abs(_two(4.0, SR.C_ | H, SR.C_ | H, n_torsions=10)["total"] - base["inter"] / 1.585) < 1e-15
    one = _two(4.0, SR.C_ | H, SR.C_ | H, weights=(0, 0, 0, 1, 0), n_torsions=2, torsion_weight=0.5)
    assert one["inter"] == base["terms"][3] and one["total"] == base["terms"][3] / 2.0
    pose = np.zeros((1, 3), np.float32)
    with_h = SR.score(pose, [SR.C_], np.array([[4, 0, 0], [1, 0, 0]], np.float32), [6, 1], [SR.C_, SR.C_])
    assert with_h["n_pairs"] == 1                                        # the hydrogen takes no part
    assert SR.score(pose, [SR.C_], np.zeros((0, 3)), [], [])["terms"].tolist() == [0.0] * 5
    assert SR.score(np.array([[np.nan, 0, 0]], np.float32), [SR.C_], [[4, 0, 0]], [6], [SR.C_])["flags"] == SR.NONFINITE
    assert SR.score(pose, [SR.C_], [[4, 0, 0]], [6], [SR.C_], lig_status=3)["flags"] == SR.UNCHECKED
    assert SR.score(pose, [SR.C_], [[4, 0, 0]], [6], [SR.C_], grid_status=6)["flags"] == SR.UNCHECKED


def test_radii_are_the_published_ones():
    from fabind_amd import scoring
    assert scoring.RADII == (1.9, 1.8, 1.7, 2.1, 2.0, 1.5, 1.8, 2.0, 2.2, 1.2) and SR.RADII[:10].tolist() == list(scoring.RADII)
    assert scoring.VINA_WEIGHTS == SR.WEIGHTS == (-0.035579, -0.005156, 0.840245, -0.035069, -0.587439)
    for z, cls in ((6, "C"), (7, "N"), (8, "O"), (15, "P"), (16, "S"), (9, "F"), (17, "Cl"), (35, "Br"), (53, "I"), (30, "metal"), (12, "metal"),
                   (5, "metal"), (14, "metal"), (34, "metal")):
        w = int(scoring.protein_types_from_elements(np.array([z]))[0])
        assert scoring.RADIUS_CLASSES[w & 15] == cls and w == SR.element_word(z), z
    assert int(scoring.protein_types_from_elements(np.array([30]))[0]) & D and not int(scoring.protein_types_from_elements(np.array([5]))[0]) & 0x70
    assert (scoring.HYDROPHOBIC, scoring.DONOR, scoring.ACCEPTOR) == (H, D, A)
    assert scoring.SCORE_FLAGS == dict(NONFINITE=SR.NONFINITE, UNCHECKED=SR.UNCHECKED)


# ------------------------------------------------------------------------------------------------ ligand typing
SINGLE, DOUBLE, TRIPLE, AROM = 4, 3, 2, 1


def _lig(z, bonds, codes, **kw):
    from fabind_amd import scoring
    bi = np.asarray(bonds, np.int64).reshape(-1, 2).T
    got = scoring.ligand_types(torch.as_tensor(bi), torch.as_tensor(np.asarray(codes, np.int64)), torch.as_tensor(np.asarray(z, np.int64)),
                               [0, len(z)], **kw).numpy()
    want = SR.ligand_types(len(z), bonds, codes, z, n_hydrogens=kw.get("n_hydrogens"), charge=kw.get("formal_charge"))
    assert got.dtype == np.int32 and got.tolist() == want.tolist(), (got, want)
    return got


def _roles(w):
    return "".join(c for c, bit in (("h", H), ("d", D), ("a", A)) if w & bit)


def test_ligand_typing_on_hand_molecules():
    eth = _lig([6, 6, 8], [(0, 1), (1, 2)], [SINGLE, SINGLE])           # ethanol
    assert [_roles(w) for w in eth] == ["h", "", "da"]
    ace = _lig([6, 6, 8, 6], [(0, 1), (1, 2), (1, 3)], [SINGLE, DOUBLE, SINGLE])      # acetone
    assert [_roles(w) for w in ace] == ["h", "", "a", "h"]
    ring = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)]
    pyr_k = _lig([7, 6, 6, 6, 6, 6], ring, [DOUBLE, SINGLE, DOUBLE, SINGLE, DOUBLE, SINGLE])      # pyridine, Kekule
    pyr_a = _lig([7, 6, 6, 6, 6, 6], ring, [AROM] * 6)                                            # pyridine, aromatic coding
    for pyr in (pyr_k, pyr_a):
        assert [_roles(w) for w in pyr] == ["a", "", "h", "h", "h", ""]
    five = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)]
    pyrrole = _lig([7, 6, 6, 6, 6], five, [SINGLE, DOUBLE, SINGLE, DOUBLE, SINGLE])               # pyrrole, Kekule: N-H
    assert _roles(pyrrole[0]) == "d"
    arom_pyrrole = _lig([7, 6, 6, 6, 6], five, [AROM] * 5)                                        # the documented limit ...
    assert _roles(arom_pyrrole[0]) == "a"
    assert _roles(_lig([7, 6, 6, 6, 6], five, [AROM] * 5, n_hydrogens=[1, 1, 1, 1, 1])[0]) == "d"  # ... and the override
    amide = _lig([6, 6, 8, 7, 6], [(0, 1), (1, 2), (1, 3), (3, 4)], [SINGLE, DOUBLE, SINGLE, SINGLE])     # N-methylacetamide
    assert [_roles(w) for w in amide] == ["h", "", "a", "d", ""]
    tma = _lig([7, 6, 6, 6], [(0, 1), (0, 2), (0, 3)], [SINGLE] * 3)                              # trimethylamine
    assert _roles(tma[0]) == "" and (tma[0] & 15) == SR.N_
    clbz = _lig([17, 6, 6, 6, 6, 6, 6], [(0, 1)] + [(1 + k, 1 + (k + 1) % 6) for k in range(6)], [SINGLE] + [AROM] * 6)   # chlorobenzene
    assert _roles(clbz[0]) == "h" and (clbz[0] & 15) == SR.CL_ and _roles(clbz[1]) == "" and _roles(clbz[3]) == "h"
    nitrile = _lig([6, 6, 7], [(0, 1), (1, 2)], [SINGLE, TRIPLE])
    assert _roles(nitrile[2]) == "a"
    ammonium = _lig([6, 7], [(0, 1)], [SINGLE], formal_charge=[0, 1])                             # methylammonium: three hydrogens
    assert _roles(ammonium[1]) == "d"
    nitro = _lig([6, 7, 8, 8], [(0, 1), (1, 2), (1, 3)], [SINGLE, DOUBLE, SINGLE], formal_charge=[0, 1, 0, -1])
    assert _roles(nitro[1]) == "" and _roles(nitro[2]) == "a" and _roles(nitro[3]) == "a"
    zinc = _lig([30, 15, 5], [], [])
    assert _roles(zinc[0]) == "d" and (zinc[0] & 15) == SR.METAL_ and _roles(zinc[1]) == "" and zinc[2] == SR.METAL_


def test_ligand_typing_ignores_direction_repeats_and_batching():
    from fabind_amd import scoring
    z = np.array([6, 6, 8, 7, 6, 6, 8, 6], np.int64)                    # N-methylacetamide and acetone in one batch
    bonds = [(0, 1), (1, 2), (1, 3), (3, 4), (5, 6), (5, 7)]
    codes = [SINGLE, DOUBLE, SINGLE, SINGLE, DOUBLE, SINGLE]
    once = _lig(z, bonds, codes)
    both = np.array(bonds + [(j, i) for i, j in bonds] + bonds[:2], np.int64).T
    got = scoring.ligand_types(torch.as_tensor(both), codes + codes + codes[:2], torch.as_tensor(z), [0, 5, 8]).numpy()
    assert got.tolist() == once.tolist()
    names = scoring.ligand_types(torch.as_tensor(np.array(bonds).T), ["SINGLE", "DOUBLE", "SINGLE", "SINGLE", "DOUBLE", "SINGLE"],
                                 torch.as_tensor(z), [0, 5, 8]).numpy()
    assert names.tolist() == once.tolist()
    with pytest.raises(ValueError):
        scoring.ligand_types(torch.as_tensor(both), codes, torch.as_tensor(z), [0, 5, 8])
    with pytest.raises(ValueError):
        scoring.ligand_types(torch.as_tensor(np.array(bonds).T), codes, torch.as_tensor(z), [0, 5, 9])


def test_hydrogen_counts_from_sdf():
    from fabind_amd import embed, scoring
    # methanol with explicit hydrogens, the hydroxyl hydrogen listed between the heavy atoms
    atoms = [("C", 0.0), ("H", 1.0), ("O", 2.0), ("H", 3.0), ("H", 4.0), ("H", 5.0)]
    bonds = [(1, 3), (1, 4), (1, 5), (1, 6), (3, 2)]
    text = "methanol\n  hand\n\n%3d%3d  0  0  0  0  0  0  0  0999 V2000\n" % (len(atoms), len(bonds))
    text += "".join("%10.4f%10.4f%10.4f %-3s 0  0  0  0  0  0  0  0  0  0  0  0\n" % (x, 0.0, 0.0, s) for s, x in atoms)
    text += "".join("%3d%3d%3d  0\n" % (a, b, 1) for a, b in bonds) + "M  END\n"
    nh = scoring.hydrogen_counts_from_sdf(text)
    mol = embed.molecule_from_sdf(text)
    assert mol["atomic_numbers"].tolist() == [6, 8] and nh.tolist() == [3, 1] and nh.dtype == np.int32
    t = scoring.ligand_types(torch.as_tensor(mol["bonds"].T), torch.as_tensor(mol["bond_codes"]), torch.as_tensor(mol["atomic_numbers"]), [0, 2],
                             n_hydrogens=nh).numpy()
    assert [_roles(w) for w in t] == ["", "da"]
    with pytest.raises(ValueError):
        scoring.hydrogen_counts_from_sdf("x\n")


# ------------------------------------------------------------------------------------------------ the protein table
_RES_ATOMS = {
    "ALA": "N CA C O CB", "ARG": "N CA C O CB CG CD NE CZ NH1 NH2", "ASN": "N CA C O CB CG OD1 ND2", "ASP": "N CA C O CB CG OD1 OD2",
    "CYS": "N CA C O CB SG", "GLN": "N CA C O CB CG CD OE1 NE2", "GLU": "N CA C O CB CG CD OE1 OE2", "GLY": "N CA C O",
    "HIS": "N CA C O CB CG ND1 CD2 CE1 NE2", "ILE": "N CA C O CB CG1 CG2 CD1", "LEU": "N CA C O CB CG CD1 CD2", "LYS": "N CA C O CB CG CD CE NZ",
    "MET": "N CA C O CB CG SD CE", "PHE": "N CA C O CB CG CD1 CD2 CE1 CE2 CZ", "PRO": "N CA C O CB CG CD", "SER": "N CA C O CB OG",
    "THR": "N CA C O CB OG1 CG2", "TRP": "N CA C O CB CG CD1 CD2 NE1 CE2 CE3 CZ2 CZ3 CH2", "TYR": "N CA C O CB CG CD1 CD2 CE1 CE2 CZ OH",
    "VAL": "N CA C O CB CG1 CG2 OXT",
}


def _pdb_line(rec, serial, name, res, resseq, xyz, element):
    return "%-6s%5d %-4s %3s A%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s" % (rec, serial, (" " + name) if len(name) < 4 else name, res, resseq,
                                                                                  xyz[0], xyz[1], xyz[2], element)


def _synthetic_pdb():
    rng = np.random.RandomState(0)
    lines, keys, serial = [], [], 1
    for k, (res, atoms) in enumerate(sorted(_RES_ATOMS.items())):
        for name in atoms.split():
            lines.append(_pdb_line("ATOM", serial, name, res, k + 1, rng.uniform(-20, 20, 3), name[0]))
            keys.append((res, name))
            serial += 1
        lines.append(_pdb_line("ATOM", serial, "H", res, k + 1, rng.uniform(-20, 20, 3), "H"))       # dropped
        serial += 1
    extra = [("ATOM", "CA", "MSE", "C"), ("ATOM", "SE", "MSE", "SE"), ("ATOM", "N", "MSE", "N"), ("ATOM", "O", "MSE", "O"),
             ("ATOM", "XX", "ALA", "C"), ("HETATM", "C1", "LIG", "C"), ("HETATM", "N1", "LIG", "N"), ("HETATM", "O1", "LIG", "O"),
             ("HETATM", "CL1", "LIG", "CL"), ("HETATM", "ZN", "ZN", "ZN"), ("HETATM", "O", "HOH", "O"), ("HETATM", "CB", "ALA", "C")]
    for rec, name, res, el in extra:
        lines.append(_pdb_line(rec, serial, name, res, 30, rng.uniform(-20, 20, 3), el))
        keys.append((rec, res, name))
        serial += 1
    return "\n".join(lines) + "\nEND\n", keys


def test_residue_table_and_fallback():
    from fabind_amd import scoring, validity
    text, keys = _synthetic_pdb()
    xyz, z, het, types = scoring.protein_types_from_pdb(text)
    x0, z0, h0 = validity.protein_atoms_from_pdb(text)
    assert xyz.tobytes() == x0.tobytes() and z.tobytes() == z0.tobytes() and het.tobytes() == h0.tobytes()
    assert xyz.dtype == x0.dtype and z.dtype == z0.dtype and het.dtype == h0.dtype and types.dtype == np.int32
    keys = [k for k in keys if k[-2] != "HOH"]                           # the water is filtered out
    assert len(keys) == len(types)
    got = {k: int(t) for k, t in zip(keys, types)}
    xw, zw, hw, tw = scoring.protein_types_from_pdb(text, keep_water=True)
    x1, z1, h1 = validity.protein_atoms_from_pdb(text, keep_water=True)
    assert xw.tobytes() == x1.tobytes() and zw.tobytes() == z1.tobytes() and hw.tobytes() == h1.tobytes() and len(tw) == len(types) + 1
    roles = lambda k: _roles(got[k])
    for res in _RES_ATOMS:
        assert roles((res, "N")) == ("" if res == "PRO" else "d"), res
        assert roles((res, "O")) == "a" and roles((res, "CA")) == "" and roles((res, "C")) == "", res
        assert (got[(res, "N")] & 15, got[(res, "O")] & 15, got[(res, "CA")] & 15) == (SR.N_, SR.O_, SR.C_)
    assert roles(("VAL", "OXT")) == "a"
    for k in (("ARG", "NE"), ("ARG", "NH1"), ("ARG", "NH2"), ("ASN", "ND2"), ("GLN", "NE2"), ("LYS", "NZ"), ("TRP", "NE1")):
        assert roles(k) == "d", k
    for k in (("HIS", "ND1"), ("HIS", "NE2"), ("SER", "OG"), ("THR", "OG1"), ("TYR", "OH")):
        assert roles(k) == "da", k
    for k in (("ASP", "OD1"), ("ASP", "OD2"), ("GLU", "OE1"), ("GLU", "OE2"), ("ASN", "OD1"), ("GLN", "OE1")):
        assert roles(k) == "a", k
    assert roles(("MET", "SD")) == "" and roles(("CYS", "SG")) == "" and got[("MET", "SD")] & 15 == SR.S_
    hydrophobic = {k for k in got if len(k) == 2 and got[k] & H}
    want = {("ALA", "CB"), ("ARG", "CB"), ("ARG", "CG"), ("ASN", "CB"), ("ASP", "CB"), ("GLN", "CB"), ("GLN", "CG"), ("GLU", "CB"), ("GLU", "CG"),
            ("HIS", "CB"), ("ILE", "CB"), ("ILE", "CG1"), ("ILE", "CG2"), ("ILE", "CD1"), ("LEU", "CB"), ("LEU", "CG"), ("LEU", "CD1"),
            ("LEU", "CD2"), ("LYS", "CB"), ("LYS", "CG"), ("LYS", "CD"), ("MET", "CB"), ("PHE", "CB"), ("PHE", "CG"), ("PHE", "CD1"),
            ("PHE", "CD2"), ("PHE", "CE1"), ("PHE", "CE2"), ("PHE", "CZ"), ("PRO", "CB"), ("PRO", "CG"), ("TRP", "CB"), ("TRP", "CG"),
            ("TRP", "CD2"), ("TRP", "CE3"), ("TRP", "CZ2"), ("TRP", "CZ3"), ("TRP", "CH2"), ("TYR", "CB"), ("TYR", "CG"), ("TYR", "CD1"),
            ("TYR", "CD2"), ("TYR", "CE1"), ("TYR", "CE2"), ("VAL", "CB"), ("VAL", "CG1"), ("VAL", "CG2"), ("THR", "CG2")}
    assert hydrophobic == want, (sorted(hydrophobic - want), sorted(want - hydrophobic))
    # outside the table: the element fallback -- carbon not hydrophobic, N without a role, O an acceptor, halogens hydrophobic, metals donors
    assert roles(("ATOM", "MSE", "CA")) == "" and roles(("ATOM", "MSE", "N")) == "" and roles(("ATOM", "MSE", "O")) == "a"
    assert got[("ATOM", "MSE", "SE")] == SR.METAL_ and roles(("ATOM", "ALA", "XX")) == ""
    assert roles(("HETATM", "LIG", "C1")) == "" and roles(("HETATM", "LIG", "N1")) == "" and roles(("HETATM", "LIG", "O1")) == "a"
    assert roles(("HETATM", "LIG", "CL1")) == "h" and roles(("HETATM", "ZN", "ZN")) == "d" and got[("HETATM", "ZN", "ZN")] & 15 == SR.METAL_
    assert roles(("HETATM", "ALA", "CB")) == ""                          # a HETATM record never reads the table
    fallback = scoring.protein_types_from_elements(z)
    outside = np.array([len(k) == 3 for k in keys])
    assert fallback.dtype == np.int32 and fallback[outside].tolist() == types[outside].tolist()
    assert [SR.element_word(v) for v in z] == fallback.tolist()
    assert scoring.protein_types_from_elements(torch.as_tensor(z)).tolist() == fallback.tolist()


# ------------------------------------------------------------------------------------------------ the wiring
def test_header_binding_and_build_list_name_the_entry_point():
    from fabind_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "fabind_hip.h")).read()
    assert "#define FABIND_ABI_VERSION 19" in hdr and _lib.ABI_VERSION == 19             # additive: the version stays
    m = re.search(r"\bint\s+fabind_pose_score\s*\(([^;{]*?)\)\s*;", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S), flags=re.S)
    assert m and m.group(1).strip().endswith("hipStream_t stream")
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES["fabind_pose_score"]) == 29
    assert "pose_score.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pose_score.hip"))
    src = open(os.path.join(build.CSRC, "pose_score.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert 'extern "C" int fabind_pose_score(' in src and "atomic" not in code and "asm" not in code
    assert "#pragma clang fp contract(off)" in src
    users = [f for f in ("kernels.py", "scoring.py") if ".fabind_pose_score(" in open(os.path.join(ROOT, "fabind_amd", f)).read()]
    assert users == ["kernels.py"]


def test_score_poses_refuses_the_host_and_the_metrics_wrapper_ranks_by_energy():
    from fabind_amd import scoring
    from fabind_amd.plus import metrics
    from fabind_amd.utils import post_optim_utils
    with pytest.raises(RuntimeError, match="HIP device only"):
        scoring.score_poses(torch.zeros(1, 2, 3), [0, 2], torch.zeros(2, dtype=torch.int32), None, torch.zeros(0, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP device only"):
        post_optim_utils.score_compound_coords_batched(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32),
                                                       None, torch.zeros(0, dtype=torch.int32))
    rmsd = torch.tensor([[1.0, 5.0], [3.0, 1.5], [0.5, 4.0]])           # [S = 3, B = 2]
    cdis = rmsd * 0.5
    energy = torch.tensor([[-3.0, -1.0], [-7.0, -9.0], [-5.0, float("nan")]])
    got = metrics.energy_sampling_metrics(rmsd, cdis, energy)
    conf = torch.where(torch.isnan(energy), torch.full_like(energy, float("-inf")), -energy)      # a pose without an energy ranks last
    want = metrics.sampling_metrics(rmsd, cdis, conf=conf)
    assert got["rmsd_mean"] == (3.0 + 1.5) / 2
    assert got.keys() == want.keys()
    for k in got:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=True), k
    valid = torch.tensor([[True, True], [False, True], [True, True]])
    got = metrics.energy_sampling_metrics(rmsd, cdis, energy, valid=valid, top_n=2)
    want = metrics.valid_sampling_metrics(rmsd, cdis, conf, valid, top_n=2)
    assert got.keys() == want.keys() and "rmsd_lt2_and_valid" in got
    for k in got:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=True), k
