"""The molecule-resident SchNet kernels (csrc/spk_schnet_mol.hip) where the operands of a matrix chain are requested ahead of it and
the chain is fenced against the scheduler: the split GEMM 2 of a pair tile in the forward, the split W2 chain of a derivative task in
the backward.  A read that is issued early must still see the data of ITS tile and ITS group -- so the cases sit on the edges of the
tiles (32 pairs), of the two teams' tile counts, of the groups and of the grid-stride loop over the groups.

Reference: the float64 oracle (oracle/spk_oracle.py) with the project's bound of 1e-5 on energies, forces and gradients, per molecule
(mol_capacity_cases.per_molecule_err); "alone" and "twice" comparisons are bit for bit.

Groups: every unit is filled up to 32 atoms or is a 32-atom cluster, so the plan keeps one group per unit (asserted on the host plan)."""
import functools

import numpy as np
import pytest
import torch

import mol_capacity_cases as C
from oracle import spk_oracle as O
from schnetpack_amd import synthetic as S

pytestmark = pytest.mark.gpu
TOL = 1e-5
COMBOS = [(L, sp, n_rbf) for L in (1, 3) for sp in (True, False) for n_rbf in (8, 20)]
# pairs inside the cutoff: one to six tiles, equal and unequal tile counts of the two teams, a last tile with one valid row and with 32
TILE_EDGE_PAIRS = (1, 31, 32, 33, 64, 65, 96, 97, 160, 161)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------
# models, runs, references
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _params(L, n_rbf):
    return O.init_schnet_params(128, L, n_rbf, C.CUTOFF), O.init_atomwise_params(128, seed=1)


@functools.lru_cache(maxsize=None)
def _model(L, n_rbf):
    from schnetpack_amd import model as M
    rep, head = _params(L, n_rbf)
    m = M.build_model("schnet", 128, L, n_rbf, C.CUTOFF)
    M.load_reference_params(m, rep, head)
    return m.to(torch.device("cuda:0")).eval()


class _split:
    """Matrix path for the length of a ``with``; afterwards the path found before."""

    def __init__(self, sp):
        self.sp = sp

    def __enter__(self):
        from schnetpack_amd import _lib
        self.sp0 = _lib.get_split()
        _lib.set_split(self.sp)

    def __exit__(self, *exc):
        from schnetpack_amd import _lib
        _lib.set_split(bool(self.sp0))


def _potential(m, batch, dev):
    """(energy, forces, tags) of the fused force call."""
    from schnetpack_amd import _lib, model as M
    _lib.profile_enable(True)
    _lib.profile_report()
    try:
        out = m(M.batch_to_inputs(batch, dev))
        res = out["energy"].detach().cpu(), out["forces"].detach().cpu()
        tags = set(_lib.profile_report())
    finally:
        _lib.profile_enable(False)
    return res[0], res[1], tags


def _two_launches(tags):
    assert tags == {"schnet_mol_fwd", "schnet_mol_bwd"}, tags


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def _reference(key, L, n_rbf):
    """float64 oracle of a named batch (once per process, never modified)."""
    rep, head = _params(L, n_rbf)
    return O.energy_and_forces("schnet", rep, head, _BATCHES[key](), L, dtype=torch.float64)


def _check(label, E, F, ref, idx_m):
    assert torch.isfinite(E).all() and torch.isfinite(F).all(), label
    err_e, mol_e = C.energy_err(E, ref["energy"])
    err_f, mol_f = C.per_molecule_err(F, ref["forces"], idx_m)
    print("%-44s energy %.3e (molecule %d)  forces %.3e (molecule %d)  bound %.0e" % (label, err_e, mol_e, err_f, mol_f, TOL))
    assert err_e < TOL and err_f < TOL, (label, err_e, err_f)


def _one_group_per_unit(b, atoms, pairs):
    plan = C.plan(b)
    assert np.diff(plan["grp_atom0"]).tolist() == list(atoms), "one group per unit"
    assert np.diff(plan["grp_pair0"]).tolist() == list(pairs), "listed pairs per group"


def _fill(systems, first_seed):
    """The systems and single atoms up to exactly 32 atoms."""
    n = sum(len(s["Z"]) for s in systems)
    return list(systems) + [C.atom(first_seed + k) for k in range(C.MAX_ATOMS - n)]


def _group_start(units):
    return np.concatenate([[0], np.cumsum([sum(len(s["Z"]) for s in u) for u in units])])


# ---------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tile_edge_batch():
    """One 32-atom group per entry of TILE_EDGE_PAIRS, every listed pair inside the cutoff."""
    b = S.collate([C.capped(32, P, 600 + P) for P in TILE_EDGE_PAIRS])
    _one_group_per_unit(b, [32] * len(TILE_EDGE_PAIRS), TILE_EDGE_PAIRS)
    return b


@functools.lru_cache(maxsize=None)
def _far_system():
    """Four atoms on a line, 5.5 A apart, with the three nearest-neighbour pairs of a 7 A list: no pair inside the cutoff."""
    R = np.array([[0.0, 0.0, 0.0], [5.5, 0.0, 0.0], [11.0, 0.0, 0.0], [16.5, 0.0, 0.0]])
    return C._system([6, 8, 1, 6], R, C._directed(np.array([0, 1, 2]), np.array([1, 2, 3])))


def _full(k):
    return C.capped(32, 384, 500 + k)


@functools.lru_cache(maxsize=None)
def _group_edge_units():
    """32 | 1 | 32 | 2 | 32 atoms, then a group whose three listed pairs all lie beyond the cutoff between two full groups."""
    return ([_full(0)], [C.atom(950)], [_full(1)], [C.dimer(530)], [_full(2)], _fill([_far_system()], 3000), [_full(3)])


@functools.lru_cache(maxsize=None)
def _group_edge_batch():
    units = _group_edge_units()
    b = S.collate([s for u in units for s in u])
    _one_group_per_unit(b, [32, 1, 32, 2, 32, 32, 32], [384, 0, 384, 1, 384, 3, 384])
    return b


@functools.lru_cache(maxsize=None)
def _skin_aspirin_batch():
    """Two aspirin frames with 7 A lists: pairs beyond the 5 A cutoff get weight zero, the padded rows of the last tile repeat the
    last pair of the list."""
    b = S.collate([C.aspirin(11, C.SKIN), C.aspirin(14, C.SKIN)])
    plan = C.plan(b)
    assert np.diff(plan["grp_atom0"]).tolist() == [21, 21]
    R, e = b["R"].numpy().astype(np.float32), plan["half"].astype(np.int64)
    d = np.sqrt(((R[b["idx_j"].numpy()[e]] - R[b["idx_i"].numpy()[e]]) ** 2).sum(-1))
    assert (d >= C.CUTOFF).any() and (d < C.CUTOFF).any() and np.diff(plan["grp_pair0"]).min() % C.TILE != 0
    return b


@functools.lru_cache(maxsize=None)
def _gradient_batch():
    """The 33- and the 97-pair group: two tiles (one row in the second) and four (one row in the fourth)."""
    b = S.collate([C.capped(32, 33, 633), C.capped(32, 97, 697)])
    _one_group_per_unit(b, [32, 32], [33, 97])
    return b


@functools.lru_cache(maxsize=None)
def _loop_batch(n_groups):
    """dimer, 32 atoms x 384 pairs, dimer, ... : n_groups groups (odd), every dimer a group of its own."""
    b = S.collate([C.dimer(530) if k % 2 == 0 else _full(0) for k in range(n_groups)])
    assert np.diff(C.plan(b)["grp_atom0"]).tolist() == [2 if k % 2 == 0 else 32 for k in range(n_groups)]
    return b


_BATCHES = {"tile_edges": _tile_edge_batch, "group_edges": _group_edge_batch, "skin_aspirin": _skin_aspirin_batch}


# ---------------------------------------------------------------------------------------------------------
# a. tile edges through the potential
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,sp,n_rbf", COMBOS)
def test_tile_edges_through_the_potential(dev, L, sp, n_rbf):
    b = _tile_edge_batch()
    with _split(sp):
        E, F, tags = _potential(_model(L, n_rbf), b, dev)
    _two_launches(tags)
    assert float(F[:32].abs().max()) > 0, "the one-pair group has forces"
    _check("tile edges L=%d split=%d n_rbf=%d" % (L, sp, n_rbf), E, F, _reference("tile_edges", L, n_rbf), b["idx_m"])


# ---------------------------------------------------------------------------------------------------------
# b. group edges
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,sp,n_rbf", COMBOS)
def test_group_edges_and_a_group_without_pairs(dev, L, sp, n_rbf):
    """Groups of 1, 2 and 32 atoms against the oracle; the group with no pair inside the cutoff has forces of exactly zero and the full
    groups either side of it are bit for bit what they are alone."""
    units, b, m = _group_edge_units(), _group_edge_batch(), _model(L, n_rbf)
    start = _group_start(units)
    with _split(sp):
        E, F, tags = _potential(m, b, dev)
        alone = [_potential(m, S.collate(list(units[k])), dev) for k in (4, 6)]
    _two_launches(tags)
    _check("group edges L=%d split=%d n_rbf=%d" % (L, sp, n_rbf), E, F, _reference("group_edges", L, n_rbf), b["idx_m"])
    assert int((F[start[5]:start[6]] != 0).sum()) == 0, "no pair inside the cutoff: no force"
    mol0 = [sum(len(u) for u in units[:k]) for k in range(len(units))]        # first molecule of every group
    for k, (E1, F1, _) in zip((4, 6), alone):
        assert float(F1.abs().max()) > 0
        assert _same(F[start[k]:start[k + 1]], F1), "forces of group %d beside the empty group" % k
        assert _same(E[mol0[k]:mol0[k] + 1], E1), "energy of group %d beside the empty group" % k


@pytest.mark.parametrize("L,sp,n_rbf", COMBOS)
def test_aspirin_with_skin_lists(dev, L, sp, n_rbf):
    b = _skin_aspirin_batch()
    with _split(sp):
        E, F, tags = _potential(_model(L, n_rbf), b, dev)
    _two_launches(tags)
    _check("aspirin 7 A lists L=%d split=%d n_rbf=%d" % (L, sp, n_rbf), E, F, _reference("skin_aspirin", L, n_rbf), b["idx_m"])


# ---------------------------------------------------------------------------------------------------------
# c. grid-stride loop over the groups
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,sp,n_rbf", COMBOS)
def test_grid_stride_loop_every_dimer_as_alone(dev, L, sp, n_rbf):
    """3 x CUs + 1 groups: every workgroup takes three or four groups, dimers and full groups in turn.  A read that is requested ahead
    of its chain must not see what the previous group left in LDS: every dimer has the bits of the dimer run alone."""
    from schnetpack_amd import _lib
    n_groups = 3 * _lib.device_info()["compute_units"] + 1
    b, m = _loop_batch(n_groups), _model(L, n_rbf)
    with _split(sp):
        E, F, tags = _potential(m, b, dev)
        E1, F1, _ = _potential(m, S.collate([C.dimer(530)]), dev)
    _two_launches(tags)
    assert float(F1.abs().max()) > 0 and torch.isfinite(F).all()
    start = np.concatenate([[0], np.cumsum([2 if k % 2 == 0 else 32 for k in range(n_groups)])])
    bad = [k for k in range(0, n_groups, 2) if not (_same(F[start[k]:start[k] + 2], F1) and _same(E[k:k + 1], E1))]
    assert not bad, "dimers that differ from the dimer alone: groups %s" % bad[:8]
    assert all(_same(F[start[k]:start[k + 1]], F[start[1]:start[2]]) for k in range(3, n_groups, 2)), "full groups differ"


# ---------------------------------------------------------------------------------------------------------
# d. representation operator: gradients to r_ij and x0
# ---------------------------------------------------------------------------------------------------------
def _representation(m, batch, dev):
    """L = sum(x * G), seeded G, through the representation operator with r_ij given: (dL/dr_ij, dL/dx0, r_ij, x0, G, tags) on the host."""
    from schnetpack_amd import _lib, model as M
    rep = m.representation
    kind, p0, p1 = rep.radial_basis.kernel_params()
    inp = M.batch_to_inputs(batch, dev)
    x0 = rep.embed(inp).detach().requires_grad_(True)
    R = inp["_positions"].detach()
    r = (R[inp["_idx_j"]] - R[inp["_idx_i"]] + inp["_offsets"]).contiguous().requires_grad_(True)
    G = torch.randn(x0.shape, generator=torch.Generator().manual_seed(5)).to(dev)
    _lib.profile_enable(True)
    _lib.profile_report()
    try:
        x = torch.ops.spk_hip.schnet(x0, r, inp["_idx_i"], inp["_idx_j"], rep.interaction_weights(), rep.n_filters, kind, p0, p1,
                                     rep.cutoff_fn.cutoff_value())
        gr, gx0 = torch.autograd.grad((x * G).sum(), [r, x0])
        tags = set(_lib.profile_report())
    finally:
        _lib.profile_enable(False)
    return gr.cpu(), gx0.cpu(), r.detach().cpu(), x0.detach().cpu(), G.cpu(), tags


def _representation_reference(L, n_rbf, batch, r, x0, G):
    """float64 oracle of the same loss on the same float32 inputs: the embedding table is replaced by the rows x0, one per atom."""
    p = {k: v.double() if v.is_floating_point() else v for k, v in _params(L, n_rbf)[0].items()}
    x0 = x0.double().requires_grad_(True)
    r = r.double().requires_grad_(True)
    p["embedding.weight"] = x0
    x = O.schnet_representation(torch.arange(x0.shape[0]), r, batch["idx_i"], batch["idx_j"], p, L)
    return torch.autograd.grad((x * G.double()).sum(), [r, x0])


@pytest.mark.parametrize("L,sp,n_rbf", COMBOS)
def test_representation_gradients_on_the_33_and_97_pair_groups(dev, L, sp, n_rbf):
    """Row sums and G tiles run in every interaction but the first here (dL/dx0 is asked for): gradients per group within 1e-5."""
    b = _gradient_batch()
    with _split(sp):
        gr, gx0, r, x0, G, tags = _representation(_model(L, n_rbf), b, dev)
    assert {"schnet_mol_fwd", "schnet_mol_bwd"} <= tags, tags
    ref_r, ref_x0 = _representation_reference(L, n_rbf, b, r, x0, G)
    idx_i = b["idx_i"].numpy()
    for g, (a0, a1) in enumerate(((0, 32), (32, 64))):
        e = torch.from_numpy((idx_i >= a0) & (idx_i < a1))
        err_r = float((gr[e].double() - ref_r[e]).abs().max() / ref_r[e].abs().max())
        err_x = float((gx0[a0:a1].double() - ref_x0[a0:a1]).abs().max() / ref_x0[a0:a1].abs().max())
        print("group %d L=%d split=%d n_rbf=%d: dL/dr_ij %.3e dL/dx0 %.3e  bound %.0e" % (g, L, sp, n_rbf, err_r, err_x, TOL))
        assert err_r < TOL and err_x < TOL, (g, err_r, err_x)


# ---------------------------------------------------------------------------------------------------------
# e. determinism
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", [True, False])
def test_two_calls_are_bit_equal_and_launch_the_two_kernels(dev, sp):
    m = _model(3, 20)
    for b in (S.molecule_batch("aspirin", 8, seed=2), _tile_edge_batch(), _group_edge_batch()):
        with _split(sp):
            E1, F1, tags = _potential(m, b, dev)
            E2, F2, _ = _potential(m, b, dev)
        _two_launches(tags)
        assert _same(E1, E2) and _same(F1, F2)
