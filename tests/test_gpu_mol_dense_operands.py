"""Dense phases of the molecule-resident SchNet kernels (csrc/spk_schnet_mol.hip: C1 / C2 of the forward, D1 / D2 of the backward).
In the split instances an activation tile that is only read as a B operand lies in LDS as the split image its writer made (row =
atom, 128 high halves | 128 low halves); the fp32 instances (``set_split(False)``) read fp32 tiles.  What can go wrong there does
not depend on the numbers but on which rows of a tile a group fills and what the group before it left behind:

a. tile occupancy -- groups of 1, 2, 21, 27 and exactly 32 atoms, one and three interactions, the two-launch potential and the
   representation operator with gradients to r_ij and x0 (``last`` false: the G tasks run in interaction 0);
b. stale rows -- three times as many groups as compute units, 32-atom groups with a dimer in every third place (``stale_rows_pattern``):
   every workgroup runs one dimer, two in three of them in LDS that still holds the rows of a 32-atom group -- asserted from the
   device's compute units and the plan; each dimer equals, bitwise, the same dimer in a batch of dimers only;
c. a group without any pair inside the cutoff between two ordinary groups;
d. two consecutive force calls give the same bits.

Reference: the float64 oracle, ``rel_err`` <= 1e-5 as in tests/test_gpu_mol.py.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

import mol_capacity_cases as C
from conftest import rel_err
from oracle import spk_oracle as O
from schnetpack_amd import synthetic as S

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _split:
    """Split-precision mode for the length of a ``with``; afterwards the mode found before."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from schnetpack_amd import _lib
        self.before = _lib.get_split()
        _lib.set_split(self.on)

    def __exit__(self, *exc):
        from schnetpack_amd import _lib
        _lib.set_split(bool(self.before))


@functools.lru_cache(maxsize=None)
def _params(n_int):
    return O.init_schnet_params(128, n_int, 20, C.CUTOFF), O.init_atomwise_params(128, seed=1)


@functools.lru_cache(maxsize=None)
def _model(n_int):
    from schnetpack_amd import model as M
    rep, head = _params(n_int)
    m = M.build_model("schnet", 128, n_int, 20, C.CUTOFF)
    M.load_reference_params(m, rep, head)
    return m.to(torch.device("cuda:0")).eval()


def _potential(m, batch, dev):
    """(energy, forces) of the two-launch potential; both molecule-resident launches must have run."""
    from schnetpack_amd import _lib, model as M
    _lib.profile_enable(True)
    _lib.profile_report()
    try:
        out = m(M.batch_to_inputs(batch, dev))
        res = out["energy"].detach().cpu(), out["forces"].detach().cpu()
        tags = set(_lib.profile_report())
    finally:
        _lib.profile_enable(False)
    assert {"schnet_mol_fwd", "schnet_mol_bwd"} <= tags and not any(t.startswith(("cfconv_", "pairwise")) for t in tags), tags
    return res


def _group_atoms(batch):
    return np.diff(C.plan(batch)["grp_atom0"]).tolist()


# ---------------------------------------------------------------------------------------------------------
# a. tile occupancy
# ---------------------------------------------------------------------------------------------------------
OCCUPANCY_GROUPS = [1, 32, 2, 32, 27, 21, 21]


@functools.lru_cache(maxsize=None)
def _occupancy_batch():
    """atom | 32-atom cluster | dimer | 32-atom cluster | three ethanol frames in one group | aspirin | aspirin: the full groups keep
    the plan from merging the atom and the dimer into a neighbour."""
    full = C.loop_system("cap384")
    b = S.collate([C.atom(24), full, C.dimer(530), full, C.ethanol(521), C.ethanol(522), C.ethanol(523), C.aspirin(11), C.aspirin(14)])
    assert _group_atoms(b) == OCCUPANCY_GROUPS
    return b


@functools.lru_cache(maxsize=None)
def _occupancy_reference(n_int):
    """float64 oracle, computed once per depth and never modified: energy and forces of the potential; for L = sum(x * G) with a
    seeded G the gradients to r_ij and to x0 (the embedding rows as a leaf)."""
    b = _occupancy_batch()
    rep, head = _params(n_int)
    pot = O.energy_and_forces("schnet", rep, head, b, n_int, dtype=torch.float64)
    p = {k: v.double() if v.is_floating_point() else v for k, v in rep.items()}
    N = int(b["Z"].shape[0])
    x0 = p["embedding.weight"][b["Z"]].clone().requires_grad_(True)
    r = O.pairwise_vectors(b["R"].double(), b["idx_i"], b["idx_j"], b["offsets"].double()).clone().requires_grad_(True)
    q = dict(p)
    q["embedding.weight"] = x0
    x = O.schnet_representation(torch.arange(N), r, b["idx_i"], b["idx_j"], q, n_int)
    G = torch.randn(N, 128, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    gr, gx0 = torch.autograd.grad((x * G).sum(), [r, x0])
    return pot["energy"], pot["forces"], G, x.detach(), gr, gx0


@pytest.mark.parametrize("sp", [True, False])
@pytest.mark.parametrize("n_int", [1, 3])
def test_tile_occupancy_potential_and_representation_gradients(dev, n_int, sp):
    from schnetpack_amd import _lib, model as M
    b = _occupancy_batch()
    e_ref, f_ref, G, x_ref, gr_ref, gx0_ref = _occupancy_reference(n_int)
    m = _model(n_int)
    figures = []
    with _split(sp):
        e, f = _potential(m, b, dev)
        figures += [("energy", rel_err(e, e_ref)), ("forces", rel_err(f, f_ref))]
        # the representation operator: gx_out is the input of D1, dL/dx0 is asked for
        rep = m.representation
        kind, p0, p1 = rep.radial_basis.kernel_params()
        inp = M.batch_to_inputs(b, dev)
        x0 = rep.embed(inp).detach().requires_grad_(True)
        r = torch.ops.spk_hip.pairwise(inp["_positions"], inp["_idx_i"], inp["_idx_j"], inp["_offsets"]).detach().requires_grad_(True)
        _lib.profile_enable(True)
        _lib.profile_report()
        try:
            x = torch.ops.spk_hip.schnet(x0, r, inp["_idx_i"], inp["_idx_j"], rep.interaction_weights(), rep.n_filters, kind, p0, p1,
                                         rep.cutoff_fn.cutoff_value())
            gr, gx0 = torch.autograd.grad((x * G.float().to(dev)).sum(), [r, x0])
            tags = set(_lib.profile_report())
        finally:
            _lib.profile_enable(False)
        assert {"schnet_mol_fwd", "schnet_mol_bwd"} <= tags, tags
        figures += [("x", rel_err(x.detach().cpu(), x_ref)), ("dL/dr_ij", rel_err(gr.cpu(), gr_ref)), ("dL/dx0", rel_err(gx0.cpu(), gx0_ref))]
    for name, err in figures:
        print("n_int=%d split=%d %-9s rel err %.3e  bound %.1e" % (n_int, sp, name, err, TOL))
    assert all(err <= TOL for _, err in figures), figures


# ---------------------------------------------------------------------------------------------------------
# b. stale rows
# ---------------------------------------------------------------------------------------------------------
def stale_rows_pattern(cus):
    """Group sizes of the stale-rows batch for a device of ``cus`` compute units.  Both launches run min(groups, cus) workgroups and
    workgroup w takes the groups w, w + cus, w + 2 cus, ...; with a 32-atom group and a dimer strictly in turn and an even number
    of compute units a workgroup would only ever see one kind.  So the period is odd: full groups with a dimer in every p-th place,
    p the smallest odd number that does not divide ``cus``, p * cus groups in all.  Then the p groups of a workgroup are one of every
    place of the period, the group ``cus`` places before a dimer is always a full one, and two dimers are never neighbours in the
    batch (the plan would merge them into one group)."""
    p = 3
    while cus % p == 0:
        p += 2
    return [2 if g % p == p - 1 else 32 for g in range(p * cus)]


def test_small_group_after_a_full_group_in_the_same_lds(dev):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sizes = stale_rows_pattern(cus)
    grid = min(len(sizes), cus)                          # workgroups of both launches
    full = C.loop_system("cap384")
    at = [g for g, n in enumerate(sizes) if n == 2]      # groups (= molecules) that are dimers
    dimers = [C.dimer(1000 + k) for k in range(len(at))]
    it = iter(dimers)
    mixed = S.collate([full if n == 32 else next(it) for n in sizes])
    alone = S.collate(dimers)
    assert _group_atoms(mixed) == sizes
    # the property under test, from the device and the plan: a dimer in a later round runs in the LDS of a 32-atom group
    stale = [g for g in at if g >= grid]
    assert all(sizes[g - grid] == 32 for g in stale) and len(stale) >= cus // 2, (cus, len(stale))
    m = _model(3)
    with _split(True):
        e_mixed, f_mixed = _potential(m, mixed, dev)
        e_alone, f_alone = _potential(m, alone, dev)
    atom0 = np.concatenate([[0], np.cumsum(sizes)])
    rows = torch.cat([torch.arange(int(atom0[g]), int(atom0[g]) + 2) for g in at])
    e_d, f_d = e_mixed[at], f_mixed[rows]
    de = float((e_d.double() - e_alone.double()).abs().max())
    df = float((f_d.double() - f_alone.double()).abs().max())
    print("%d compute units, %d groups, %d dimers of which %d follow a 32-atom group in their workgroup; against the dimers alone: "
          "max |dE| %.3e  max |dF| %.3e  (both must be 0)" % (cus, len(sizes), len(at), len(stale), de, df))
    assert torch.equal(e_d, e_alone) and torch.equal(f_d, f_alone)
    assert float(f_alone.abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------
# c. a group without any pair inside the cutoff
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", [True, False])
def test_group_with_every_pair_beyond_the_cutoff_between_ordinary_groups(dev, sp):
    """O and H 6 A apart with their pair listed (a list with a skin): a group of its own whose only pair gives exactly zero.  Asserted
    are its zero forces, the oracle's energy of two isolated atoms, and its neighbours bit for bit as without it (which route through
    the kernels the group takes -- dropped from the tiles or a tile of weight zero -- is not observed here)."""
    far = {"Z": [8, 1], "R": np.array([[0.0, 0.0, 0.0], [6.0, 0.0, 0.0]]), "idx_i": np.array([0, 1]), "idx_j": np.array([1, 0])}
    left, right = C.loop_system("cap384"), C.capped(32, 353, 230)
    with_far, without = S.collate([left, far, right]), S.collate([left, right])
    assert _group_atoms(with_far) == [32, 2, 32] and _group_atoms(without) == [32, 32]
    rep, head = _params(3)
    ref = O.energy_and_forces("schnet", rep, head, with_far, 3, dtype=torch.float64)
    m = _model(3)
    with _split(sp):
        e, f = _potential(m, with_far, dev)
        e0, f0 = _potential(m, without, dev)
    err_e, err_f = rel_err(e, ref["energy"]), rel_err(f, ref["forces"])
    err_iso = abs(float(e[1]) - float(ref["energy"][1])) / abs(float(ref["energy"][1]))
    print("split=%d rel err energy %.3e forces %.3e, isolated-atom energy %.3e  bound %.1e; max |F| on the far pair %.3e" % (
        sp, err_e, err_f, err_iso, TOL, float(f[32:34].abs().max())))
    assert float(ref["forces"][32:34].abs().max()) == 0.0                   # the reference agrees: isolated atoms
    assert err_e <= TOL and err_f <= TOL and err_iso <= TOL
    assert float(f[32:34].abs().max()) == 0.0
    assert torch.equal(e[[0, 2]], e0) and torch.equal(torch.cat([f[:32], f[34:]]), f0)


# ---------------------------------------------------------------------------------------------------------
# d. repeatability
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", [True, False])
def test_two_consecutive_force_calls_give_the_same_bits(dev, sp):
    b = S.collate([C.aspirin(11), C.aspirin(14)])
    assert _group_atoms(b) == [21, 21]
    m = _model(3)
    with _split(sp):
        e1, f1 = _potential(m, b, dev)
        e2, f2 = _potential(m, b, dev)
    assert torch.equal(e1, e2) and torch.equal(f1, f2)
