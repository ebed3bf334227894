"""The two ends of the molecule-resident SchNet launches (csrc/spk_schnet_mol.hip): the group set-up and the energy head.  In the
split instances the head's weights are staged into the LDS images of the filter network by the team that idles in the last phase
C1 (outnet.0.weight as a split A-operand image of H / 32 row tiles, both biases and outnet.1.weight beside it), x_L is written once
more as a split image, and the head GEMM runs on the split path; the fp32 instances (``set_split(False)``) keep the fp32 path.  What
can go wrong depends on the head's width, on which rows a group fills and on what the group before left in LDS:

a. head widths 32 / 64 / 96 / 128 with shifted softplus and SiLU, biases that are NOT zero, one and three interactions, split on and
   off, on groups of 1, 2, 21, 27 and exactly 32 atoms;
b. three molecules in one group: per-molecule energies on the plain-store route and on the atomic route of the same launches;
c. stale LDS: three times as many groups as compute units, 32-atom groups with a dimer in every third place, a head of four row tiles;
   every dimer equals, bitwise, the same dimer in a batch of dimers only;
d. a group without a pair inside the cutoff between two ordinary groups; a list with a 2 A skin (compaction drops pairs);
e. two consecutive force calls give the same bits;
f. the representation operator without the head: gradients to r_ij and x0.

Reference: the float64 oracle, ``rel_err`` <= 1e-5 as in tests/test_gpu_mol.py.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

import mol_capacity_cases as C
from conftest import rel_err
from oracle import spk_oracle as O
from schnetpack_amd import synthetic as S
from test_gpu_mol_dense_operands import (_group_atoms, _model, _occupancy_batch, _occupancy_reference, _params, _potential, _split,
                                         stale_rows_pattern)

pytestmark = pytest.mark.gpu
TOL = 1e-5
ACTS = {"ssp": O.shifted_softplus, "silu": O.silu}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------
# heads of any covered width: seeded weights, biases away from zero (the default initialisation has zero biases)
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _head_params(H):
    g = torch.Generator().manual_seed(100 + H)
    lim1, lim2 = (6.0 / (128 + H)) ** 0.5, (6.0 / (H + 1)) ** 0.5
    return {"outnet.0.weight": (2 * torch.rand(H, 128, generator=g) - 1) * lim1, "outnet.0.bias": 0.2 * torch.randn(H, generator=g),
            "outnet.1.weight": (2 * torch.rand(1, H, generator=g) - 1) * lim2, "outnet.1.bias": 0.3 + 0.1 * torch.randn(1, generator=g)}


@functools.lru_cache(maxsize=None)
def _head_model(n_int, H, act):
    from schnetpack_amd import model as M
    from schnetpack_amd.nn.activations import shifted_softplus
    fn = shifted_softplus if act == "ssp" else torch.nn.functional.silu
    rep = M.SchNet(128, n_int, M.GaussianRBF(20, C.CUTOFF), M.CosineCutoff(C.CUTOFF))
    m = M.NeuralNetworkPotential(rep, input_modules=[M.PairwiseDistances()],
                                 output_modules=[M.Atomwise(n_in=128, n_hidden=H, activation=fn, output_key=M.properties.energy), M.Forces()])
    M.load_reference_params(m, _params(n_int)[0], _head_params(H))
    return m.to(torch.device("cuda:0")).eval()


@functools.lru_cache(maxsize=None)
def _representation64(n_int):
    """float64 representation of the occupancy batch with its graph (computed once per depth; the heads differentiate through it)."""
    b = _occupancy_batch()
    p = {k: v.double() if v.is_floating_point() else v for k, v in _params(n_int)[0].items()}
    R = b["R"].detach().double().clone().requires_grad_(True)
    r = O.pairwise_vectors(R, b["idx_i"], b["idx_j"], b["offsets"].double())
    return R, O.schnet_representation(b["Z"], r, b["idx_i"], b["idx_j"], p, n_int)


@functools.lru_cache(maxsize=None)
def _head_reference(n_int, H, act):
    b = _occupancy_batch()
    R, x = _representation64(n_int)
    hp = {k: v.double() for k, v in _head_params(H).items()}
    y = O.dense(O.dense(x, hp["outnet.0.weight"], hp["outnet.0.bias"], ACTS[act]), hp["outnet.1.weight"], hp["outnet.1.bias"])
    E = O.scatter_add(y, b["idx_m"], int(b["n_mol"])).squeeze(-1)
    (g,) = torch.autograd.grad(E.sum(), [R], retain_graph=True)
    return E.detach(), -g


@pytest.mark.parametrize("sp", [True, False])
@pytest.mark.parametrize("n_int", [1, 3])
@pytest.mark.parametrize("act", ["ssp", "silu"])
@pytest.mark.parametrize("H", [32, 64, 96, 128])
def test_head_widths_and_activations_on_every_tile_occupancy(dev, H, act, n_int, sp):
    b = _occupancy_batch()
    e_ref, f_ref = _head_reference(n_int, H, act)
    m = _head_model(n_int, H, act)
    with _split(sp):
        e, f = _potential(m, b, dev)          # (asserts that both molecule-resident launches ran)
    err_e, err_f = rel_err(e, e_ref), rel_err(f, f_ref)
    print("H=%d %s n_int=%d split=%d groups %s: rel err energy %.3e forces %.3e  bound %.1e" % (H, act, n_int, sp, _group_atoms(b), err_e, err_f, TOL))
    assert err_e <= TOL and err_f <= TOL


# ---------------------------------------------------------------------------------------------------------
# b. several molecules in one group
# ---------------------------------------------------------------------------------------------------------
def test_three_molecules_in_one_group_on_the_store_and_the_atomic_route(dev):
    """Three ethanol frames share a group.  The forces route knows that every molecule lies inside one group and stores the energies;
    the autograd route of the same operator accumulates them with one atomic per (group, molecule).  Same launches, same reference."""
    b = S.collate([C.ethanol(521), C.ethanol(522), C.ethanol(523)])
    assert _group_atoms(b) == [27] and int(b["n_mol"]) == 3
    rep, head = _params(3)
    ref = O.energy_and_forces("schnet", rep, head, b, 3, dtype=torch.float64)
    m = _model(3)                         # the default head: 64 hidden units, SiLU
    figures = []
    try:
        with _split(True):
            for route, forces_route in (("store", True), ("atomic", False)):
                m._potential_forces = forces_route
                e, f = _potential(m, b, dev)
                figures.append((route, rel_err(e, ref["energy"]), rel_err(f, ref["forces"])))
                print("%-6s route: per-molecule energies %s against %s, rel err energy %.3e forces %.3e  bound %.1e" % (
                    route, e.tolist(), ref["energy"].tolist(), figures[-1][1], figures[-1][2], TOL))
    finally:
        m._potential_forces = True
    assert all(ee <= TOL and fe <= TOL for _, ee, fe in figures), figures


# ---------------------------------------------------------------------------------------------------------
# c. stale LDS
# ---------------------------------------------------------------------------------------------------------
def test_dimer_after_a_full_group_with_a_head_of_four_row_tiles(dev):
    """The head images live where the next group's set-up stages filter weights, and the split x_L in a tile the next group's pair
    tiles overwrite: a dimer that follows a 32-atom group in its workgroup must not see any of it."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sizes = stale_rows_pattern(cus)
    grid = min(len(sizes), cus)
    full = C.loop_system("cap384")
    at = [g for g, n in enumerate(sizes) if n == 2]
    dimers = [C.dimer(2000 + k) for k in range(len(at))]
    it = iter(dimers)
    mixed = S.collate([full if n == 32 else next(it) for n in sizes])
    alone = S.collate(dimers)
    assert _group_atoms(mixed) == sizes
    stale = [g for g in at if g >= grid]
    assert all(sizes[g - grid] == 32 for g in stale) and len(stale) >= cus // 2, (cus, len(stale))
    m = _head_model(3, 128, "ssp")
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
    assert float(f_alone.abs().max()) > 0.0 and float(e_alone.abs().min()) > 0.0


# ---------------------------------------------------------------------------------------------------------
# d. empty and skinned lists
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", [True, False])
def test_group_without_a_pair_inside_the_cutoff_and_a_skinned_list(dev, sp):
    far = {"Z": [8, 1], "R": np.array([[0.0, 0.0, 0.0], [6.0, 0.0, 0.0]]), "idx_i": np.array([0, 1]), "idx_j": np.array([1, 0])}
    left, right = C.loop_system("cap384"), C.capped(32, 353, 230)
    with_far, without = S.collate([left, far, right]), S.collate([left, right])
    assert _group_atoms(with_far) == [32, 2, 32] and _group_atoms(without) == [32, 32]
    skinned = S.collate([C.aspirin(11, rc=C.SKIN), C.aspirin(14, rc=C.SKIN)])       # 7 A lists, 5 A model cutoff: compaction drops pairs
    d = (skinned["R"][skinned["idx_j"]] - skinned["R"][skinned["idx_i"]]).norm(dim=1)
    assert _group_atoms(skinned) == [21, 21] and int((d >= C.CUTOFF).sum()) > 0
    m = _head_model(3, 96, "ssp")
    with _split(sp):
        e, f = _potential(m, with_far, dev)
        e0, f0 = _potential(m, without, dev)
        es, fs = _potential(m, skinned, dev)
    # references: the 96-wide ssp head on the float64 representation of each batch
    def reference(b):
        p = {k: v.double() if v.is_floating_point() else v for k, v in _params(3)[0].items()}
        hp = {k: v.double() for k, v in _head_params(96).items()}
        R = b["R"].detach().double().clone().requires_grad_(True)
        x = O.schnet_representation(b["Z"], O.pairwise_vectors(R, b["idx_i"], b["idx_j"], b["offsets"].double()), b["idx_i"], b["idx_j"], p, 3)
        y = O.dense(O.dense(x, hp["outnet.0.weight"], hp["outnet.0.bias"], O.shifted_softplus), hp["outnet.1.weight"], hp["outnet.1.bias"])
        E = O.scatter_add(y, b["idx_m"], int(b["n_mol"])).squeeze(-1)
        (g,) = torch.autograd.grad(E.sum(), [R])
        return E.detach(), -g
    e_ref, f_ref = reference(with_far)
    es_ref, fs_ref = reference(skinned)
    figures = [("far: energy", rel_err(e, e_ref)), ("far: forces", rel_err(f, f_ref)), ("skin: energy", rel_err(es, es_ref)), ("skin: forces", rel_err(fs, fs_ref))]
    for name, err in figures:
        print("split=%d %-13s rel err %.3e  bound %.1e" % (sp, name, err, TOL))
    print("max |F| on the far pair %.3e (must be 0)" % float(f[32:34].abs().max()))
    assert float(f_ref[32:34].abs().max()) == 0.0
    assert all(err <= TOL for _, err in figures), figures
    assert float(f[32:34].abs().max()) == 0.0
    assert torch.equal(e[[0, 2]], e0) and torch.equal(torch.cat([f[:32], f[34:]]), f0)


# ---------------------------------------------------------------------------------------------------------
# e. repeatability
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", [True, False])
def test_two_consecutive_force_calls_are_bitwise_equal(dev, sp):
    b = _occupancy_batch()
    m = _head_model(3, 128, "silu")
    with _split(sp):
        e1, f1 = _potential(m, b, dev)
        e2, f2 = _potential(m, b, dev)
    print("split=%d max |dE| %.3e max |dF| %.3e (both must be 0)" % (sp, float((e1 - e2).abs().max()), float((f1 - f2).abs().max())))
    assert torch.equal(e1, e2) and torch.equal(f1, f2)


# ---------------------------------------------------------------------------------------------------------
# f. the representation operator: no head, features given, dL/dx0 asked for
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", [True, False])
@pytest.mark.parametrize("n_int", [1, 3])
def test_representation_operator_without_the_head(dev, n_int, sp):
    from schnetpack_amd import _lib, model as M
    b = _occupancy_batch()
    _, _, G, x_ref, gr_ref, gx0_ref = _occupancy_reference(n_int)
    rep = _model(n_int).representation
    kind, p0, p1 = rep.radial_basis.kernel_params()
    inp = M.batch_to_inputs(b, dev)
    with _split(sp):
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
    figures = [("x", rel_err(x.detach().cpu(), x_ref)), ("dL/dr_ij", rel_err(gr.cpu(), gr_ref)), ("dL/dx0", rel_err(gx0.cpu(), gx0_ref))]
    for name, err in figures:
        print("n_int=%d split=%d %-9s rel err %.3e  bound %.1e" % (n_int, sp, name, err, TOL))
    assert all(err <= TOL for _, err in figures), figures
