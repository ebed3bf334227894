"""The molecule-resident SchNet kernels (csrc/spk_schnet_mol.hip) with the two teams of the forward half a round apart and the sigmoids
of the backward and the energy head on the hardware transcendentals (spk_fast_sigmoid: rcp(1 + exp2(-log2(e) x)), no select).

Phase A of the forward runs in half-steps: team 0 alternates hidden(0), tile(0), hidden(2), ...; team 1 runs in2f, hidden(1), tile(1), ...
Which team finishes last, and whether the other one idles through the last half-step, depends on the tile count and its parity -- so
the cases are one to twelve tiles with a last tile of one row and of 32, groups without a tile at all, and the grid-stride loop in
which a short group follows a long one.  The sigmoid cases drive the pre-activations to where exp2 overflows.

Reference: the float64 oracle (oracle/spk_oracle.py) with the project's bound of 1e-5 on energies, forces and gradients, per molecule
(mol_capacity_cases.per_molecule_err); "alone" and "twice" comparisons are bit for bit.  Batches, models and references are built the
way tests/test_gpu_mol_matrix_overlap.py builds them (its helpers are imported, its caches shared)."""
import functools

import numpy as np
import pytest
import torch

import mol_capacity_cases as C
import test_gpu_mol_matrix_overlap as T
from oracle import spk_oracle as O
from schnetpack_amd import synthetic as S

pytestmark = pytest.mark.gpu
TOL = 1e-5
COMBOS = T.COMBOS          # one / three interactions x split on / off x n_rbf 8 / 20
# pairs inside the cutoff -> tiles of team 0 / team 1 -> half-steps the teams need (the loop takes the larger):
#   1: 1/0 -> 2/1     32: 1/0 -> 2/1     33: 1/1 -> 2/3     64: 1/1 -> 2/3     65: 2/1 -> 4/3     96: 2/1 -> 4/3
#  97: 2/2 -> 4/5    128: 2/2 -> 4/5    129: 3/2 -> 6/5    160: 3/2 -> 6/5    161: 3/3 -> 6/7    384: 6/6 -> 12/13
SCHEDULE_EDGE_PAIRS = (1, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 384)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _schedule_edge_batch():
    """One 32-atom group per entry of SCHEDULE_EDGE_PAIRS, every listed pair inside the cutoff."""
    b = S.collate([C.capped(32, P, 600 + P) for P in SCHEDULE_EDGE_PAIRS])
    T._one_group_per_unit(b, [32] * len(SCHEDULE_EDGE_PAIRS), SCHEDULE_EDGE_PAIRS)
    return b


@functools.lru_cache(maxsize=None)
def _schedule_edge_reference(L, n_rbf):
    rep, head = T._params(L, n_rbf)
    return O.energy_and_forces("schnet", rep, head, _schedule_edge_batch(), L, dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------------
# a. schedule edges
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,sp,n_rbf", COMBOS)
def test_schedule_edges_through_the_potential(dev, L, sp, n_rbf):
    b = _schedule_edge_batch()
    with T._split(sp):
        E, F, tags = T._potential(T._model(L, n_rbf), b, dev)
    T._two_launches(tags)
    assert float(F[:32].abs().max()) > 0, "the one-pair group has forces"
    T._check("schedule edges L=%d split=%d n_rbf=%d" % (L, sp, n_rbf), E, F, _schedule_edge_reference(L, n_rbf), b["idx_m"])


@pytest.mark.parametrize("L,sp,n_rbf", COMBOS)
def test_schedule_edges_representation_gradients(dev, L, sp, n_rbf):
    """dL/dr_ij and dL/dx0 of the representation operator on the 33-pair group (team 1 ends the loop) and the 97-pair group."""
    b = T._gradient_batch()
    with T._split(sp):
        gr, gx0, r, x0, G, tags = T._representation(T._model(L, n_rbf), b, dev)
    assert {"schnet_mol_fwd", "schnet_mol_bwd"} <= tags, tags
    ref_r, ref_x0 = T._representation_reference(L, n_rbf, b, r, x0, G)
    idx_i = b["idx_i"].numpy()
    for g, (a0, a1) in enumerate(((0, 32), (32, 64))):
        e = torch.from_numpy((idx_i >= a0) & (idx_i < a1))
        assert torch.isfinite(gr).all() and torch.isfinite(gx0).all()
        err_r = float((gr[e].double() - ref_r[e]).abs().max() / ref_r[e].abs().max())
        err_x = float((gx0[a0:a1].double() - ref_x0[a0:a1]).abs().max() / ref_x0[a0:a1].abs().max())
        print("group %d L=%d split=%d n_rbf=%d: dL/dr_ij %.3e dL/dx0 %.3e  bound %.0e" % (g, L, sp, n_rbf, err_r, err_x, TOL))
        assert err_r < TOL and err_x < TOL, (g, err_r, err_x)


# ---------------------------------------------------------------------------------------------------------
# b. degenerate groups: no tile at all (one half-step: in2f alone), one pair
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,sp,n_rbf", COMBOS)
def test_groups_without_a_tile_between_full_groups(dev, L, sp, n_rbf):
    """32 | 1 | 32 | 2 | 32 atoms, then a group whose listed pairs all lie beyond the cutoff, then 32: the group without a pair inside
    the cutoff has forces of exactly zero, and the full groups either side of it are bit for bit what they are alone."""
    units, b, m = T._group_edge_units(), T._group_edge_batch(), T._model(L, n_rbf)
    start = T._group_start(units)
    with T._split(sp):
        E, F, tags = T._potential(m, b, dev)
        alone = [T._potential(m, S.collate(list(units[k])), dev) for k in (4, 6)]
    T._two_launches(tags)
    T._check("degenerate groups L=%d split=%d n_rbf=%d" % (L, sp, n_rbf), E, F, T._reference("group_edges", L, n_rbf), b["idx_m"])
    assert int((F[start[5]:start[6]] != 0).sum()) == 0, "no pair inside the cutoff: no force"
    assert int((F[start[1]:start[2]] != 0).sum()) == 0, "a single atom: no force"
    assert float(F[start[3]:start[4]].abs().max()) > 0, "the dimer has forces"
    mol0 = [sum(len(u) for u in units[:k]) for k in range(len(units))]        # first molecule of every group
    for k, (E1, F1, _) in zip((4, 6), alone):
        assert float(F1.abs().max()) > 0
        assert T._same(F[start[k]:start[k + 1]], F1), "forces of group %d beside the empty group" % k
        assert T._same(E[mol0[k]:mol0[k] + 1], E1), "energy of group %d beside the empty group" % k


# ---------------------------------------------------------------------------------------------------------
# c. grid-stride loop over the groups
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", [True, False])
def test_group_loop_dimers_as_alone_and_two_calls_bit_equal(dev, sp):
    """3 x CUs + 1 groups, dimers (2 half-steps) and 32-atom groups of 384 pairs (13 half-steps) in turn: every workgroup takes three or
    four of them.  Every dimer has the bits of the dimer alone, and a second call has the bits of the first."""
    from schnetpack_amd import _lib
    n_groups = 3 * _lib.device_info()["compute_units"] + 1
    b, m = T._loop_batch(n_groups), T._model(3, 20)
    with T._split(sp):
        E, F, tags = T._potential(m, b, dev)
        E2, F2, _ = T._potential(m, b, dev)
        E1, F1, _ = T._potential(m, S.collate([C.dimer(530)]), dev)
    T._two_launches(tags)
    assert float(F1.abs().max()) > 0 and torch.isfinite(F).all()
    assert T._same(E, E2) and T._same(F, F2), "two consecutive calls differ"
    start = np.concatenate([[0], np.cumsum([2 if k % 2 == 0 else 32 for k in range(n_groups)])])
    bad = [k for k in range(0, n_groups, 2) if not (T._same(F[start[k]:start[k] + 2], F1) and T._same(E[k:k + 1], E1))]
    assert not bad, "dimers that differ from the dimer alone: groups %s" % bad[:8]
    assert all(T._same(F[start[k]:start[k + 1]], F[start[1]:start[2]]) for k in range(3, n_groups, 2)), "full groups differ"


# ---------------------------------------------------------------------------------------------------------
# d. range of the select-free sigmoid
# ---------------------------------------------------------------------------------------------------------
# Bands of 16 hidden channels in the bias of the first filter-network layer (the argument of the derivative task's sigmoid) and in
# f2out.0.bias (pre3: the argument of D1's sigmoid), in every interaction; the other channels as seeded (zero).
#   channels 16-31: -100.  exp2(+144) overflows to +inf and the sigmoid must come out as +0; ssp(-100) = -ln 2, harmless to the model.
#   channels  0-15: +100 as first tried leaves the float64 reference finite but takes max |F| from 0.90 to 1.6e6 eV/A (the hidden
#                   activations of the band are ~100 and multiply through three interactions): not a model of the unscaled one's order.
#                   Halved until the reference alone has max |F| within a decade of the unscaled model's: 50 -> 3.1e5, 25 -> 4.0e4,
#                   12.5 -> 5.7e3, 6.25 -> 6.9e2, 3.125 -> 69, 1.5625 -> 4.4.  The negative band stays at -100 (with it alone: 2.7).
BAND_NEG, BAND_POS = -100.0, 1.5625


@functools.lru_cache(maxsize=None)
def _banded_params():
    rep = {k: v.clone() for k, v in O.init_schnet_params(128, 3, 20, C.CUTOFF).items()}
    for l in range(3):
        for key in ("interactions.%d.filter_network.0.bias" % l, "interactions.%d.f2out.0.bias" % l):
            rep[key][0:16] = BAND_POS
            rep[key][16:32] = BAND_NEG
    return rep, O.init_atomwise_params(128, seed=1)


@functools.lru_cache(maxsize=None)
def _banded_batch():
    b = S.collate([C.aspirin(11)])
    assert np.diff(C.plan(b)["grp_atom0"]).tolist() == [21]
    return b


@functools.lru_cache(maxsize=None)
def _banded_reference():
    """float64 oracle of the banded model -- confirmed on the host, before anything runs on the device, to be finite and of the
    unscaled model's order."""
    rep, head = _banded_params()
    ref = O.energy_and_forces("schnet", rep, head, _banded_batch(), 3, dtype=torch.float64)
    plain = O.energy_and_forces("schnet", *T._params(3, 20), _banded_batch(), 3, dtype=torch.float64)
    fmax, fmax0 = float(ref["forces"].abs().max()), float(plain["forces"].abs().max())
    assert torch.isfinite(ref["forces"]).all() and torch.isfinite(ref["energy"]).all()
    assert 0.1 * fmax0 < fmax < 10.0 * fmax0, (fmax, fmax0)
    return ref


@pytest.mark.parametrize("sp", [True, False])
def test_sigmoid_range_bands_of_saturated_channels(dev, sp):
    from schnetpack_amd import model as M
    ref, b = _banded_reference(), _banded_batch()
    rep, head = _banded_params()
    m = M.build_model("schnet", 128, 3, 20, C.CUTOFF)
    M.load_reference_params(m, rep, head)
    m = m.to(dev).eval()
    with T._split(sp):
        E, F, tags = T._potential(m, b, dev)
    T._two_launches(tags)
    T._check("sigmoid range split=%d" % sp, E, F, ref, b["idx_m"])
