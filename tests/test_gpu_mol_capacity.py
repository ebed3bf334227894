"""The molecule-resident kernels (csrc/spk_schnet_mol.hip, csrc/spk_painn_mol.hip) at the edges of their group capacity: 32 atoms
(``kMaxGroupAtoms`` / ``MAX_GROUP_ATOMS``), 384 pairs (``ML_MAXPAIRS``; ``PM_MAXEDGES`` = 768 directed), twelve 32-pair tiles, six
interactions (``ML_MAXL`` / ``PM_MAXL``).  The inputs are the seeded cases of tests/mol_capacity_cases.py (checked on the CPU by
tests/test_mol_capacity_cases.py: they have the counts their names say, and the float32 oracle is within 3e-6 of the float64 oracle on
them).

Metric: per MOLECULE, max|got - ref| / max|ref| over the atoms of that molecule (energies: |E - E_ref| / |E_ref|) -- a wrong small
group cannot hide behind a large neighbour.  Against the float64 oracle the bound is the project's 1e-5; between
two device paths on the same batch it is 2e-6 on representations and energies and 5e-6 on forces, as in tests/test_gpu_mol.py and
tests/test_gpu_painn_mol.py.  Every figure is printed before it is asserted (``pytest -s``)."""
import functools
import os

import numpy as np
import pytest
import torch

import mol_capacity_cases as C
from oracle import spk_oracle as O
from schnetpack_amd import synthetic as S

pytestmark = pytest.mark.gpu
TOL = 1e-5                      # against the float64 oracle
X_REP, X_FORCES = 2e-6, 5e-6    # between two device paths
KINDS = ["schnet", "painn"]
GENERAL_TAGS = ("cfconv_", "pairwise", "atomwise_")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------
# models, routes, references
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _params(kind, n_int, n_rbf, radial):
    init = O.init_schnet_params if kind == "schnet" else O.init_painn_params
    return init(128, n_int, n_rbf, C.CUTOFF, radial=radial), O.init_atomwise_params(128, seed=1)


@functools.lru_cache(maxsize=4)
def _model(kind, n_int, n_rbf, radial):
    from schnetpack_amd import model as M
    rep, head = _params(kind, n_int, n_rbf, radial)
    m = M.build_model(kind, 128, n_int, n_rbf, C.CUTOFF, radial)
    M.load_reference_params(m, rep, head)
    return m.to(torch.device("cuda:0")).eval()


def _run(kind, batch, dev, route="potential", n_int=3, n_rbf=20, radial="gaussian"):
    """route: "potential" -- the standard potential as one operator (two launches where the list is eligible); "modules" -- module by
    module (``_potential = False``: representation operator, Atomwise, Forces); "general" -- the general driver (SchNet:
    VARIANT_MFMA_DIRECTED never takes the molecule path; PaiNN: SPK_NO_PAINN_MOL).  Returns (dict of host tensors, set of tags)."""
    from schnetpack_amd import _lib, model as M
    m = _model(kind, n_int, n_rbf, radial)
    flags = (m._potential, m._potential_forces)
    assert flags == (True, True)
    try:
        if route == "modules":
            m._potential, m._potential_forces = False, False
        elif route == "general":
            if kind == "schnet":
                _lib.set_variant(_lib.VARIANT_MFMA_DIRECTED)
            else:
                os.environ["SPK_NO_PAINN_MOL"] = "1"
        _lib.profile_enable(True)
        _lib.profile_report()
        inp = M.batch_to_inputs(batch, dev)
        out = m(inp)
        res = {"energy": out["energy"].detach().cpu(), "forces": out["forces"].detach().cpu(),
               "scalar_representation": inp["scalar_representation"].detach().cpu()}
        if kind == "painn":
            res["vector_representation"] = inp["vector_representation"].detach().cpu()
        tags = set(_lib.profile_report())
    finally:
        _lib.profile_enable(False)
        _lib.set_variant(_lib.VARIANT_AUTO)
        os.environ.pop("SPK_NO_PAINN_MOL", None)
        m._potential, m._potential_forces = flags
    return res, tags


@functools.lru_cache(maxsize=None)
def _reference(name, kind, n_int=3, n_rbf=20, radial="gaussian"):
    """float64 oracle of a named case (computed once per process; never modified)."""
    rep, head = _params(kind, n_int, n_rbf, radial)
    return O.energy_and_forces(kind, rep, head, C.batch(name), n_int, dtype=torch.float64, need_rep=True)


def _atom_keys(kind):
    return ["forces", "scalar_representation"] + (["vector_representation"] if kind == "painn" else [])


def _compare(label, got, ref, idx_m, kind, bounds):
    """Per-molecule errors of energy / forces / representation(s); prints every figure, returns the failures."""
    bad = []
    for key in _atom_keys(kind) + ["energy"]:
        err, mol = C.energy_err(got[key], ref[key]) if key == "energy" else C.per_molecule_err(got[key], ref[key], idx_m)
        bound = bounds["forces" if key == "forces" else "other"]
        print("%-46s %-22s worst molecule %4d  err %.3e  bound %.1e" % (label, key, mol, err, bound))
        if not err < bound:
            bad.append((label, key, mol, err, bound))
    return bad


def _oracle_bounds():
    return {"forces": TOL, "other": TOL}


def _cross_bounds():
    return {"forces": X_FORCES, "other": X_REP}


def _mol_tags(kind):
    return {kind + "_mol_fwd", kind + "_mol_bwd"}


def _assert_two_launches(tags, kind):
    assert _mol_tags(kind) <= tags, tags
    assert not any(t.startswith(GENERAL_TAGS) for t in tags), tags


def _assert_no_molecule_kernel(tags):
    assert not any("_mol_" in t for t in tags), tags


# ---------------------------------------------------------------------------------------------------------
# a. capacity parity
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", C.CAPACITY_CASES)
def test_capacity_parity(dev, name, kind):
    """Groups of 28 / 32 atoms with 378 ... 384 pairs (12 tiles with tails of 26, 0, 31 and 1 pairs; 11 tiles), 32 atoms with 33 pairs,
    groups merged to exactly 32 atoms and groups one atom too large to merge: module by module and as the two-launch potential, against
    the float64 oracle and against the general driver."""
    b = C.batch(name)
    ref = _reference(name, kind)
    pot, tags_pot = _run(kind, b, dev, "potential")
    mod, tags_mod = _run(kind, b, dev, "modules")
    gen, tags_gen = _run(kind, b, dev, "general")
    _assert_two_launches(tags_pot, kind)
    assert _mol_tags(kind) <= tags_mod and any(t.startswith("atomwise_") for t in tags_mod), tags_mod
    _assert_no_molecule_kernel(tags_gen)
    bad = _compare("%s/%s potential vs float64" % (name, kind), pot, ref, b["idx_m"], kind, _oracle_bounds())
    bad += _compare("%s/%s modules vs float64" % (name, kind), mod, ref, b["idx_m"], kind, _oracle_bounds())
    bad += _compare("%s/%s general vs float64" % (name, kind), gen, ref, b["idx_m"], kind, _oracle_bounds())
    bad += _compare("%s/%s potential vs general" % (name, kind), pot, gen, b["idx_m"], kind, _cross_bounds())
    bad += _compare("%s/%s modules vs general" % (name, kind), mod, gen, b["idx_m"], kind, _cross_bounds())
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# b. both sides of the boundary
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,molecule_path", [("cap384", True), ("over385", False), ("merge32", True), ("over33", False)])
def test_eligibility_flips_between_384_and_385_pairs_and_between_32_and_33_atoms(dev, name, molecule_path, kind):
    """384 pairs (ML_MAXPAIRS; 2 x 384 = PM_MAXEDGES) and 32 atoms (kMaxGroupAtoms) run the molecule kernels; one pair or one atom
    more anywhere in the batch and the whole batch takes the general driver -- with the same results."""
    b = C.batch(name)
    meta = C.plan(b)["meta"]
    assert (meta[3] > 0 and meta[4] <= C.MAX_ATOMS and meta[5] <= C.MAX_PAIRS) == molecule_path
    res, tags = _run(kind, b, dev, "potential")
    if molecule_path:
        _assert_two_launches(tags, kind)
    else:
        _assert_no_molecule_kernel(tags)
    bad = _compare("%s/%s potential vs float64" % (name, kind), res, _reference(name, kind), b["idx_m"], kind, _oracle_bounds())
    mod, tags_mod = _run(kind, b, dev, "modules")
    if molecule_path:
        assert _mol_tags(kind) <= tags_mod, tags_mod
    else:
        _assert_no_molecule_kernel(tags_mod)
    bad += _compare("%s/%s modules vs float64" % (name, kind), mod, _reference(name, kind), b["idx_m"], kind, _oracle_bounds())
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# c. basis and depth at capacity
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rbf,radial", [(8, "gaussian"), (9, "gaussian"), (24, "gaussian"), (25, "gaussian"), (32, "gaussian"), (16, "bessel")])
def test_schnet_basis_sizes_at_capacity(dev, n_rbf, radial):
    """Every KPB instance (ceil(n_rbf / 8) = 1 ... 4) and both sides of each 8-wide block on 32 atoms x 384 pairs; the backward is
    molecule-resident exactly when n_rbf <= 24."""
    b = C.batch("cap384")
    res, tags = _run("schnet", b, dev, "potential", 3, n_rbf, radial)
    assert "schnet_mol_fwd" in tags and not any(t.startswith("cfconv_fwd") for t in tags), tags
    assert ("schnet_mol_bwd" in tags) == (n_rbf <= 24), tags
    if n_rbf <= 24:
        _assert_two_launches(tags, "schnet")
    bad = _compare("cap384/schnet n_rbf=%d %s vs float64" % (n_rbf, radial), res, _reference("cap384", "schnet", 3, n_rbf, radial),
                   b["idx_m"], "schnet", _oracle_bounds())
    assert not bad, bad


@pytest.mark.parametrize("n_rbf,radial,molecule_path", [(8, "gaussian", True), (12, "gaussian", True), (16, "gaussian", True), (20, "gaussian", True),
                                                         (16, "bessel", True), (24, "gaussian", False)])
def test_painn_basis_sizes_at_capacity(dev, n_rbf, radial, molecule_path):
    """The four instances of the PaiNN kernels (n_rbf = 8, 12, 16, 20) on 32 atoms x 768 directed edges; n_rbf = 24 has no instance
    and takes the general driver."""
    b = C.batch("cap384")
    res, tags = _run("painn", b, dev, "potential", 3, n_rbf, radial)
    if molecule_path:
        _assert_two_launches(tags, "painn")
    else:
        _assert_no_molecule_kernel(tags)
    bad = _compare("cap384/painn n_rbf=%d %s vs float64" % (n_rbf, radial), res, _reference("cap384", "painn", 3, n_rbf, radial),
                   b["idx_m"], "painn", _oracle_bounds())
    assert not bad, bad


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_int,molecule_path", [(6, True), (7, False)])
def test_depth_at_capacity(dev, n_int, molecule_path, kind):
    """Six interactions (ML_MAXL / PM_MAXL: the offsets into the saved tensors scale with the depth) run the molecule kernels on full
    groups, seven take the general driver."""
    b = C.batch("cap384")
    res, tags = _run(kind, b, dev, "potential", n_int)
    if molecule_path:
        _assert_two_launches(tags, kind)
    else:
        _assert_no_molecule_kernel(tags)
    bad = _compare("cap384/%s n_interactions=%d vs float64" % (kind, n_int), res, _reference("cap384", kind, n_int), b["idx_m"], kind,
                   _oracle_bounds())
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# d. skin list at capacity
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_skin_list_at_capacity(dev, kind):
    """A 7 A list with 384 listed pairs per 32-atom group, 27 % of them beyond the 5 A model cutoff: the per-call compaction shrinks
    a FULL pair-record array.  Finite, equal to the float64 oracle on the same skin list and to the run on the exact list."""
    bs, be = C.batch("skin384"), C.batch("skin384_exact")
    assert C.plan(bs)["meta"][5] == C.MAX_PAIRS and bs["idx_i"].shape[0] > be["idx_i"].shape[0]
    skin, tags = _run(kind, bs, dev, "potential")
    exact, tags_e = _run(kind, be, dev, "potential")
    _assert_two_launches(tags, kind)
    _assert_two_launches(tags_e, kind)
    for key, v in skin.items():
        assert torch.isfinite(v).all(), key
    bad = _compare("skin384/%s vs float64 (skin list)" % kind, skin, _reference("skin384", kind), bs["idx_m"], kind, _oracle_bounds())
    bad += _compare("skin384/%s vs float64 (exact list)" % kind, exact, _reference("skin384_exact", kind), be["idx_m"], kind, _oracle_bounds())
    bad += _compare("skin384/%s skin list vs exact list" % kind, skin, exact, bs["idx_m"], kind, _cross_bounds())
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# e. the workgroup loop over unlike groups
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loop_reference(kind):
    """float64 oracle of loop_mixed: every unit of a kind is the same instance and molecules do not interact, so the oracle runs on
    one system per label and its rows are laid out in batch order."""
    systems, labels = C.loop_systems()
    distinct = sorted(set(labels))
    small = S.collate([C.loop_system(l) for l in distinct])
    rep, head = _params(kind, 3, 20, "gaussian")
    r = O.energy_and_forces(kind, rep, head, small, 3, dtype=torch.float64, need_rep=True)
    start = np.concatenate([[0], np.cumsum([len(C.loop_system(l)["Z"]) for l in distinct])])
    where = {l: k for k, l in enumerate(distinct)}
    rows = torch.from_numpy(np.concatenate([np.arange(start[where[l]], start[where[l] + 1]) for l in labels]))
    out = {key: r[key][rows] for key in _atom_keys(kind)}
    out["energy"] = r["energy"][torch.tensor([where[l] for l in labels])]
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_workgroup_loop_over_unlike_groups(dev, kind):
    """More groups than compute units, full and tiny groups in a seeded order: a workgroup meets a dimer after a 384-pair group and
    the reverse.  Every molecule within the bound, and what a group gets does not depend on what its workgroup processed before: the
    representation rows of every 32-atom / 28-atom cluster and of every group with a dimer are BIT-equal to that group's rows as the
    first group of a three-group batch (PaiNN: the forces too; SchNet's backward adds per-pair sums in task order: 2e-6)."""
    from schnetpack_amd import _lib
    b = C.batch("loop_mixed")
    groups = C.loop_groups()
    cus = _lib.device_info()["compute_units"]
    assert len(groups) >= 1.25 * cus, (len(groups), cus)
    res, tags = _run(kind, b, dev, "potential")
    _assert_two_launches(tags, kind)
    bad = _compare("loop_mixed/%s vs float64" % kind, res, _loop_reference(kind), b["idx_m"], kind, _oracle_bounds())
    assert not bad, bad
    start = np.concatenate([[0], np.cumsum([len(s["Z"]) for s in C.case("loop_mixed")])])
    alone, checked, worst_f = {}, 0, 0.0
    for s0, s1, labels in groups:
        if labels not in (("cap384",), ("full28",)) and "dimer" not in labels:
            continue
        if labels not in alone:
            alone[labels], tags_a = _run(kind, S.collate(C.loop_group_alone(labels)), dev, "potential")
            _assert_two_launches(tags_a, kind)
        a0, a1 = int(start[s0]), int(start[s1])
        first = alone[labels]
        for key in ["scalar_representation"] + (["vector_representation", "forces"] if kind == "painn" else []):
            assert torch.equal(res[key][a0:a1], first[key][:a1 - a0]), (key, labels, s0)
        if kind == "schnet":
            f, f0 = res["forces"][a0:a1].double(), first["forces"][:a1 - a0].double()
            e = float((f - f0).abs().max() / f0.abs().max())
            worst_f = max(worst_f, e)
            assert e < 2e-6, (labels, s0, e)
        checked += 1
    print("loop_mixed/%s: %d groups, %d compared bit for bit with %d first-group runs; worst force difference %.3e"
          % (kind, len(groups), checked, len(alone), worst_f))
    assert checked >= 0.3 * len(groups)


# ---------------------------------------------------------------------------------------------------------
# f. the two implementations of the plan agree
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.ALL_CASES)
def test_device_plan_equals_host_plan(dev, name):
    """``data.host_plan`` (numpy, in the collate workers) and the plan the operator library derives on the device from fresh index
    tensors (csrc/spk_torch.cpp) are two implementations of the same greedy merge: same arrays, same counts."""
    from schnetpack_amd import torchops  # noqa: F401
    b = C.batch(name)
    host = C.plan(b)
    n_atoms = int(b["Z"].shape[0])
    idx_i, idx_j = b["idx_i"].to(dev).clone(), b["idx_j"].to(dev).clone()
    R = b["R"].to(dev).float()
    r_ij = (R[idx_j] - R[idx_i] + b["offsets"].to(dev).float()).contiguous()      # the device pairs (i, j) with (j, i) through r_ji == -r_ij
    arrs = torch.ops.spk_hip.edge_plan_arrays(idx_i, idx_j, n_atoms, r_ij)
    rowptr, rev, half, edge_pair, grp_atom0, grp_pair0, _, meta = arrs[:8]
    meta = meta.cpu().numpy()
    assert meta[:6].tolist() == host["meta"][:6].tolist() and meta[7] == host["meta"][7], (meta, host["meta"])
    for what, t in (("rowptr", rowptr), ("rev", rev), ("half", half), ("edge_pair", edge_pair), ("grp_atom0", grp_atom0), ("grp_pair0", grp_pair0)):
        got = t.cpu().numpy()
        assert got.dtype == host[what].dtype and np.array_equal(got, host[what]), what
