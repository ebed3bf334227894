"""GPU: the point-charge electrostatics kernels (csrc/spk_coulomb.hip, csrc/spk_ewald.hip) through every route -- the C ABI, the operators
``torch.ops.spk_hip.coulomb`` / ``ewald_recip`` with autograd, the module mirrors inside a module-by-module model, a model whose charges are
predicted by ``DipoleMoment`` -- against the float64 fixture the reference's own code produced (tests/golden/electrostatic_cases.npz,
tests/make_electrostatic_golden.py).

Tolerance: the project's parity contract, 1e-5 relative in the max-norm, on E, F, dE/dq and W, with no extra margin; the
reference's own float32 gap on these cases is below a quarter of it (``gap_*`` in the fixture).  On E1, the exact rock-salt lattice, the forces
vanish by symmetry and are measured against max|E| / a.  Every test prints what it measured."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import electrostatic_oracle as EO  # noqa: E402

from schnetpack_amd import _lib, model as M, properties  # noqa: E402
from schnetpack_amd import atomistic as A  # noqa: E402
from schnetpack_amd._lib import fptr, iptr, stream  # noqa: E402
from schnetpack_amd.nn import CosineCutoff, GaussianRBF, SwitchFunction, fallback  # noqa: E402
from schnetpack_amd.representation import PaiNN, SchNet  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1.0e-5
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "electrostatic_cases.npz"))
COULOMB = [(c, v) for c, vs in EO.COULOMB.items() for v in vs]
EWALD = [(c, v) for c, vs in EO.EWALD.items() for v in vs]
EWALD_HIP = [(c, v) for c, v in EWALD if c != "E4"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    return torch.device("cuda", 0)


def rel(x, ref, scale=None):
    ref = ref.detach().cpu().double().numpy() if torch.is_tensor(ref) else np.asarray(ref, dtype=np.float64)
    x = x.detach().cpu().double().numpy() if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)
    scale = np.abs(ref).max() if scale is None else scale
    return float(np.abs(x.reshape(ref.shape) - ref).max() / (scale if scale > 0 else 1.0))


def force_scale(case, v):
    return float(np.abs(v["E"]).max() / 5.64) if case == "E1" else None


_CASES = {}


def case(tag, dev):
    """Fixture case on the device (built once, never modified)."""
    if tag not in _CASES:
        c = EO.case_inputs(GOLD, tag)
        t = lambda k: torch.tensor(c[k], dtype=torch.float32 if c[k].dtype.kind == "f" else torch.long, device=dev)
        inp = {properties.R: t("R"), properties.cell: t("cell"), properties.offsets: t("offsets"), properties.idx_i: t("idx_i"),
               properties.idx_j: t("idx_j"), properties.idx_m: t("idx_m"), properties.partial_charges: t("q"), "_n_molecules": int(c["n_mol"])}
        _CASES[tag] = (c, inp)
    return _CASES[tag]


def fresh(inp):
    """A per-test copy of the input dict whose positions and charges are new leaves."""
    out = dict(inp)
    out[properties.R] = inp[properties.R].clone().requires_grad_()
    out[properties.partial_charges] = inp[properties.partial_charges].clone().requires_grad_()
    return out


def check(tag, route, v, E, F, gq, W=None, fscale=None):
    eE, eF, eq = rel(E, v["E"]), rel(F, v["F"], fscale), rel(gq, v["dEdq"])
    eW = rel(W, v["W"]) if W is not None else 0.0
    print("electrostatics %-16s %-9s E %.3e F %.3e dEdq %.3e W %.3e" % (tag, route, eE, eF, eq, eW))
    assert eE < TOL and eF < TOL and eq < TOL and eW < TOL, (tag, route, eE, eF, eq, eW)


def coulomb_mirror(var, dev, lr=False):
    pot = A.DampedCoulombPotential(SwitchFunction(*EO.SWITCH)) if var.startswith("damped") else A.CoulombPotential()
    return A.EnergyCoulomb("eV", "Ang", pot, "e", use_neighbors_lr=lr, cutoff=EO.CUTOFF if var.endswith("_cut") else None).to(dev).eval()


def ewald_mirror(tag, v, dev, lr=False):
    unit = ("Ha", "Bohr") if tag == "E1" else ("eV", "Ang")
    return A.EnergyEwald(float(v["alpha"]), int(v["k_max"]), unit[0], unit[1], "e", use_neighbors_lr=lr,
                         screening_fn=SwitchFunction(*EO.SWITCH) if bool(v["screened"]) else None).to(dev).eval()


# ----------------------------------------------------------------------------------------------------------------- C ABI
def c_abi_pairs(inp, n_mol, prm, dev, gE=None):
    """spk_coulomb_fwd_f32 / _bwd_f32 and the landing of gr on atoms and virial: (E, E_atom, gR, gq, W, plan)."""
    from schnetpack_amd import ops
    L = _lib.lib()
    R, off, idx_m, q = inp[properties.R], inp[properties.offsets], inp[properties.idx_m], inp[properties.partial_charges]
    N = R.shape[0]
    r = torch.ops.spk_hip.pairwise(R, inp[properties.idx_i], inp[properties.idx_j], off)
    plan = ops.EdgePlan(inp[properties.idx_i], inp[properties.idx_j], N, r)
    ws = torch.empty(int(L.spk_coulomb_workspace_bytes(plan.graph(), n_mol)), dtype=torch.uint8, device=dev)
    E, Ea, phi = torch.full((n_mol,), 7.0, device=dev), torch.full((N,), 7.0, device=dev), torch.full((N,), 7.0, device=dev)
    _lib.check(L.spk_coulomb_fwd_f32(fptr(r), fptr(q), plan.graph(), iptr(idx_m), n_mol, fptr(prm), fptr(E), fptr(Ea), fptr(phi),
                                     ctypes.c_void_p(ws.data_ptr()), stream()))
    gE = torch.ones(n_mol, device=dev) if gE is None else gE
    gr, gq = torch.full_like(r, 7.0), torch.full((N,), 7.0, device=dev)
    _lib.check(L.spk_coulomb_bwd_f32(fptr(gE), fptr(r), fptr(q), fptr(phi), plan.graph(), iptr(idx_m), n_mol, fptr(prm), fptr(gr), fptr(gq),
                                     ctypes.c_void_p(ws.data_ptr()), stream()))
    gR = torch.empty(N, 3, device=dev)
    _lib.check(L.spk_pairwise_bwd_graph_f32(fptr(gr), plan.graph(), fptr(gR), stream()))
    W = torch.empty(n_mol, 3, 3, device=dev)
    vws = torch.empty(int(L.spk_edge_virial_workspace_bytes(plan.graph(), n_mol, 0)), dtype=torch.uint8, device=dev)
    _lib.check(L.spk_edge_virial_f32(fptr(gr), fptr(R), fptr(off), plan.graph(), iptr(idx_m), n_mol, fptr(W), None, ctypes.c_void_p(vws.data_ptr()), stream()))
    return E, Ea, gR, gq, W, plan


def c_abi_recip(inp, n_mol, v, dev):
    """spk_ewald_recip_fwd_f32 / _bwd_f32: (E, coeffs, gR, gq)."""
    L = _lib.lib()
    R, idx_m, q, cell = inp[properties.R], inp[properties.idx_m], inp[properties.partial_charges], inp[properties.cell]
    N, k_max = R.shape[0], int(v["k_max"])
    kv = torch.tensor(EO.kvecs(k_max), dtype=torch.float32, device=dev)
    K = kv.shape[0]
    prm = torch.tensor([float(v["ke"]), float(v["alpha"])], dtype=torch.float32, device=dev)
    ws = torch.empty(int(L.spk_ewald_workspace_bytes(N, K, n_mol)), dtype=torch.uint8, device=dev)
    E, coef = torch.full((n_mol,), 7.0, device=dev), torch.full((n_mol, K, 2), 7.0, device=dev)
    _lib.check(L.spk_ewald_recip_fwd_f32(fptr(R), fptr(q), fptr(cell), iptr(idx_m), N, n_mol, fptr(kv), K, k_max, fptr(prm), fptr(E), fptr(coef),
                                         ctypes.c_void_p(ws.data_ptr()), stream()))
    gR, gq = torch.full((N, 3), 7.0, device=dev), torch.full((N,), 7.0, device=dev)
    _lib.check(L.spk_ewald_recip_bwd_f32(fptr(torch.ones(n_mol, device=dev)), fptr(R), fptr(q), fptr(cell), iptr(idx_m), N, n_mol, fptr(kv), K, k_max,
                                         fptr(prm), fptr(coef), fptr(gR), fptr(gq), ctypes.c_void_p(ws.data_ptr()), stream()))
    return E, coef, gR, gq


@pytest.mark.parametrize("tag,var", COULOMB)
def test_c_abi_coulomb(dev, tag, var):
    (c, inp), v = case(tag, dev), EO.variant(GOLD, tag, var)
    prm = torch.tensor(EO.params8(v), dtype=torch.float32, device=dev)
    E, Ea, gR, gq, W, plan = c_abi_pairs(inp, int(c["n_mol"]), prm, dev)
    assert (plan.sorted and plan.symmetric) == (tag != "C2")
    check("%s/%s" % (tag, var), "c-abi", v, E, -gR, gq, W if tag == "C3" else None)
    zero = np.nonzero(c["q"] == 0)[0]
    assert bool((Ea[torch.tensor(zero, device=dev)] == 0).all())                      # an atom without charge: an exact zero
    assert rel(torch.zeros(int(c["n_mol"]), device=dev).index_add(0, inp[properties.idx_m], Ea), v["E"]) < TOL


@pytest.mark.parametrize("tag,var", EWALD_HIP)
def test_c_abi_ewald(dev, tag, var):
    (c, inp), v = case(tag, dev), EO.variant(GOLD, tag, var)
    n_mol = int(c["n_mol"])
    Er, _, gRr, gqr, _, _ = c_abi_pairs(inp, n_mol, torch.tensor(EO.params8(v), dtype=torch.float32, device=dev), dev)
    Ek, coef, gRk, gqk = c_abi_recip(inp, n_mol, v, dev)
    eR, eK = rel(Er, v["E_real"]), rel(Ek, v["E_rec"])
    print("electrostatics %s/%s c-abi E_real %.3e E_rec %.3e" % (tag, var, eR, eK))
    assert eR < TOL and eK < TOL
    check("%s/%s" % (tag, var), "c-abi", v, Er + Ek, -(gRr + gRk), gqr + gqk, fscale=force_scale(tag, v))
    if tag == "E1":
        madelung = -float(Er[0] + Ek[0]) * 5.64 / 8.0
        print("electrostatics E1 Madelung constant %.7f" % madelung)
        assert abs(madelung / EO.MADELUNG_NACL - 1.0) < TOL


def test_c_abi_incoming_gradient_scales_every_molecule(dev):
    (c, inp), v = case("E3", dev), EO.variant(GOLD, "E3", "k2")
    n_mol = int(c["n_mol"])
    w = torch.tensor([2.0, -0.5, 4.0], device=dev)                                    # powers of two: the scaling is exact in float32
    prm = torch.tensor(EO.params8(v), dtype=torch.float32, device=dev)
    _, _, gR1, gq1, _, _ = c_abi_pairs(inp, n_mol, prm, dev)
    _, _, gR2, gq2, _, _ = c_abi_pairs(inp, n_mol, prm, dev, gE=w)
    wa = w[inp[properties.idx_m]]
    assert torch.equal(gR2, gR1 * wa[:, None]) and torch.equal(gq2, gq1 * wa)


# ----------------------------------------------------------------------------------------------------------------- operators
@pytest.mark.parametrize("tag,var", COULOMB)
def test_coulomb_operator_with_autograd(dev, tag, var):
    (c, inp), v = case(tag, dev), EO.variant(GOLD, tag, var)
    x = fresh(inp)
    prm = torch.tensor(EO.params8(v), dtype=torch.float32, device=dev)
    r = torch.ops.spk_hip.pairwise(x[properties.R], x[properties.idx_i], x[properties.idx_j], x[properties.offsets])
    E = torch.ops.spk_hip.coulomb(r, x[properties.partial_charges], x[properties.idx_i], x[properties.idx_j], x[properties.idx_m], int(c["n_mol"]), prm)[0]
    gR, gq = torch.autograd.grad(E.sum(), [x[properties.R], x[properties.partial_charges]])
    check("%s/%s" % (tag, var), "operator", v, E, -gR, gq)


@pytest.mark.parametrize("tag,var", EWALD_HIP)
def test_ewald_operators_with_autograd(dev, tag, var):
    (c, inp), v = case(tag, dev), EO.variant(GOLD, tag, var)
    x = fresh(inp)
    n_mol, q = int(c["n_mol"]), x[properties.partial_charges]
    r = torch.ops.spk_hip.pairwise(x[properties.R], x[properties.idx_i], x[properties.idx_j], x[properties.offsets])
    Er = torch.ops.spk_hip.coulomb(r, q, x[properties.idx_i], x[properties.idx_j], x[properties.idx_m], n_mol,
                                   torch.tensor(EO.params8(v), dtype=torch.float32, device=dev))[0]
    kv = torch.tensor(EO.kvecs(int(v["k_max"])), dtype=torch.float32, device=dev)
    Ek = torch.ops.spk_hip.ewald_recip(x[properties.R], q, x[properties.cell], x[properties.idx_m], n_mol, kv,
                                       torch.tensor([float(v["ke"]), float(v["alpha"])], dtype=torch.float32, device=dev))[0]
    gR, gq = torch.autograd.grad((Er + Ek).sum(), [x[properties.R], q])
    check("%s/%s" % (tag, var), "operator", v, Er + Ek, -gR, gq, fscale=force_scale(tag, v))


def test_recorded_backward_raises(dev):
    (c, inp), v = case("E2", dev), EO.variant(GOLD, "E2", "k4")
    for which in ("coulomb", "ewald_recip"):
        x = fresh(inp)
        r = torch.ops.spk_hip.pairwise(x[properties.R], x[properties.idx_i], x[properties.idx_j], x[properties.offsets])
        if which == "coulomb":
            E = torch.ops.spk_hip.coulomb(r, x[properties.partial_charges], x[properties.idx_i], x[properties.idx_j], x[properties.idx_m], 1,
                                          torch.tensor(EO.params8(v), dtype=torch.float32, device=dev))[0]
        else:
            E = torch.ops.spk_hip.ewald_recip(x[properties.R], x[properties.partial_charges], x[properties.cell], x[properties.idx_m], 1,
                                              torch.tensor(EO.kvecs(4), dtype=torch.float32, device=dev),
                                              torch.tensor([float(v["ke"]), float(v["alpha"])], dtype=torch.float32, device=dev))[0]
        with pytest.raises(RuntimeError, match="first-order gradients"):
            torch.autograd.grad(E.sum(), [x[properties.R]], create_graph=True)


def test_two_calls_give_identical_bits(dev):
    (c, inp), v = case("E3", dev), EO.variant(GOLD, "E3", "k2")
    n_mol = int(c["n_mol"])
    prm = torch.tensor(EO.params8(v), dtype=torch.float32, device=dev)
    a, b = c_abi_pairs(inp, n_mol, prm, dev), c_abi_pairs(inp, n_mol, prm, dev)
    assert a[5].sorted and a[5].symmetric and all(torch.equal(x, y) for x, y in zip(a[:5], b[:5]))
    a, b = c_abi_recip(inp, n_mol, v, dev), c_abi_recip(inp, n_mol, v, dev)
    assert all(torch.equal(x, y) for x, y in zip(a, b))                              # E, the S(k) coefficients, gR, gq


def test_empty_list_gives_zeros(dev):
    inp = {properties.R: torch.randn(4, 3, device=dev), properties.offsets: torch.zeros(0, 3, device=dev), properties.idx_i: torch.zeros(0, dtype=torch.long, device=dev),
           properties.idx_j: torch.zeros(0, dtype=torch.long, device=dev), properties.idx_m: torch.tensor([0, 0, 1, 1], device=dev),
           properties.partial_charges: torch.tensor([0.5, -0.5, 0.3, 0.1], device=dev), "_n_molecules": 2}
    x = fresh(inp)
    mod = coulomb_mirror("damped_cut", dev)
    out = mod(A.PairwiseDistances()(x))
    gR, gq = torch.autograd.grad(out["e"].sum(), [x[properties.R], x[properties.partial_charges]], allow_unused=True)
    assert bool((out["e"] == 0).all()) and (gR is None or bool((gR == 0).all())) and bool((gq == 0).all())
    torch.cuda.synchronize()


def test_pad_atoms_and_out_of_range_indices(dev):
    """Pad atoms (q = 0) stacked on one point contribute exact zeros, also to the gradients; a neighbour index outside the atoms never reaches
    the kernels through a plan (which reports it; the kernels clamp such an index for the read all the same)."""
    (c, inp), v = case("C1", dev), EO.variant(GOLD, "C1", "damped_cut")
    N, n_mol = len(c["R"]), int(c["n_mol"])
    R = torch.cat([inp[properties.R], torch.zeros(3, 3, device=dev)])
    q = torch.cat([inp[properties.partial_charges], torch.zeros(3, device=dev)])
    pad = torch.tensor([[N, N + 1], [N, N + 2], [N + 1, N], [N + 1, N + 2], [N + 2, N], [N + 2, N + 1]], device=dev)
    x = {properties.R: R, properties.partial_charges: q, properties.idx_i: torch.cat([inp[properties.idx_i], pad[:, 0]]),
         properties.idx_j: torch.cat([inp[properties.idx_j], pad[:, 1]]), properties.offsets: torch.cat([inp[properties.offsets], torch.zeros(6, 3, device=dev)]),
         properties.idx_m: torch.cat([inp[properties.idx_m], torch.full((3,), n_mol - 1, device=dev)])}
    prm = torch.tensor(EO.params8(v), dtype=torch.float32, device=dev)
    E, Ea, gR, gq, W, _ = c_abi_pairs(x, n_mol, prm, dev)
    assert bool((Ea[N:] == 0).all()) and bool((gR[N:] == 0).all()) and bool(torch.isfinite(gR).all()) and bool((gq[N:] == 0).all())
    check("C1/pad", "c-abi", v, E, -gR[:N], gq[:N])
    bad = dict(inp)
    bad[properties.idx_j] = inp[properties.idx_j].clone()
    bad[properties.idx_j][5] = N + 1000
    with pytest.raises(_lib.SpkHipError, match="out of range"):
        c_abi_pairs(bad, n_mol, prm, dev)
    torch.cuda.synchronize()


def test_zero_volume_cell_gives_nan_for_that_molecule_only(dev):
    (c, inp), v = case("E3", dev), EO.variant(GOLD, "E3", "k1")
    x = dict(inp)
    x[properties.cell] = inp[properties.cell].clone()
    x[properties.cell][1, 2] = x[properties.cell][1, 1]
    Ek, _, gR, gq = c_abi_recip(x, 3, v, dev)
    m = inp[properties.idx_m]
    assert bool(torch.isnan(Ek[1])) and bool(torch.isfinite(Ek[[0, 2]]).all()) and rel(Ek[[0, 2]], v["E_rec"][[0, 2]]) < TOL
    assert bool(torch.isnan(gR[m == 1]).all()) and bool(torch.isfinite(gR[m != 1]).all()) and bool(torch.isfinite(gq[m != 1]).all())


# ----------------------------------------------------------------------------------------------------------------- modules and models
def schnet_model(term, dev, strain=False, stress=False):
    """The PhysNet-style composition: the full list goes to the long-range keys for the electrostatic term, SchNet sees the pairs within 5 A."""
    rep = SchNet(64, 2, GaussianRBF(20, 5.0), CosineCutoff(5.0))
    ins = ([A.Strain()] if strain else []) + [A.PairwiseDistances(), A.FilterShortRange(5.0)]
    return M.NeuralNetworkPotential(rep, input_modules=ins, output_modules=[term, A.Forces(calc_stress=stress, energy_key="e")]).to(dev).eval()


def model_inputs(inp, n_atoms):
    x = dict(inp)
    x[properties.Z] = torch.full((n_atoms,), 6, dtype=torch.long, device=inp[properties.R].device)
    x[properties.R] = inp[properties.R].clone()
    return x


@pytest.mark.parametrize("tag,var", [cv for cv in COULOMB if cv[0] != "C2"])      # (C2, the half list, is a case of the pair kernels, not of SchNet)
def test_energy_coulomb_inside_a_schnet_model_with_charges_from_the_batch(dev, tag, var):
    (c, inp), v = case(tag, dev), EO.variant(GOLD, tag, var)
    model = schnet_model(coulomb_mirror(var, dev, lr=True), dev, strain=tag == "C3", stress=tag == "C3")
    assert M.classify_potential(model) == 0
    n0 = fallback.fallback_count()
    out = model(model_inputs(inp, len(c["R"])))
    assert fallback.fallback_count() == n0                                            # the operator route
    eE, eF = rel(out["e"], v["E"]), rel(out["forces"], v["F"])
    eW = 0.0
    if tag == "C3":
        cell = torch.tensor(c["cell"])
        eW = rel(out["stress"].cpu().double() * torch.linalg.det(cell)[:, None, None], v["W"])
    print("electrostatics %s/%s model E %.3e F %.3e W %.3e" % (tag, var, eE, eF, eW))
    assert eE < TOL and eF < TOL and eW < TOL


@pytest.mark.parametrize("tag,var", EWALD)
def test_energy_ewald_inside_a_schnet_model_with_charges_from_the_batch(dev, tag, var):
    (c, inp), v = case(tag, dev), EO.variant(GOLD, tag, var)
    model = schnet_model(ewald_mirror(tag, v, dev, lr=True), dev)
    n0 = fallback.fallback_count()
    out = model(model_inputs(inp, len(c["R"])))
    assert (fallback.fallback_count() > n0) == (tag == "E4")                          # k_max beyond the cap: the ATen route, on the device
    eE, eF = rel(out["e"], v["E"]), rel(out["forces"], v["F"], force_scale(tag, v))
    print("electrostatics %s/%s model E %.3e F %.3e" % (tag, var, eE, eF))
    assert eE < TOL and eF < TOL
    if tag == "E1":
        assert abs(-float(out["e"][0].detach()) * 5.64 / 8.0 / EO.MADELUNG_NACL - 1.0) < TOL


def small_batch(dev, dtype=torch.float32):
    """The 5- and the 17-atom cluster of C1 with a 5 A list: inputs of a PaiNN model."""
    c = EO.case_inputs(GOLD, "C1")
    sel = c["idx_m"] < 2
    n = int(sel.sum())
    R = c["R"][:n]
    keep = (c["idx_i"] < n) & (c["idx_j"] < n)
    ii, jj = c["idx_i"][keep], c["idx_j"][keep]
    near = np.linalg.norm(R[jj] - R[ii], axis=1) < 5.0
    ii, jj = ii[near], jj[near]
    Z = np.asarray([1, 6, 8])[np.arange(n) % 3]
    return {properties.Z: torch.tensor(Z, device=dev), properties.R: torch.tensor(R, dtype=dtype, device=dev),
            properties.offsets: torch.zeros(len(ii), 3, dtype=dtype, device=dev), properties.idx_i: torch.tensor(ii, device=dev),
            properties.idx_j: torch.tensor(jj, device=dev), properties.idx_m: torch.tensor(c["idx_m"][:n], device=dev), "_n_molecules": 2}


def charge_model(dev):
    torch.manual_seed(11)
    rep = PaiNN(64, 2, GaussianRBF(20, 5.0), CosineCutoff(5.0))
    outs = [A.DipoleMoment(64, use_vector_representation=True, return_charges=True),
            A.EnergyCoulomb("eV", "Ang", A.DampedCoulombPotential(SwitchFunction(*EO.SWITCH)), "e_el", use_neighbors_lr=False),
            A.Atomwise(64, output_key="e_nn"), A.Aggregation(["e_nn", "e_el"], "energy"), A.Forces()]
    return M.NeuralNetworkPotential(rep, input_modules=[A.PairwiseDistances()], output_modules=outs).to(dev).eval()


def test_forces_through_predicted_charges_in_eval_mode(dev):
    model = charge_model(dev)
    assert M.classify_potential(model) == 0 and model.output_modules[0]._charges_differentiable
    out = model(small_batch(dev))
    ref = model.double()(small_batch(dev, torch.float64))                             # every mirror on its ATen route, float64
    model.float()
    eE, eF, eq = rel(out["energy"], ref["energy"]), rel(out["forces"], ref["forces"]), rel(out["partial_charges"], ref["partial_charges"])
    # the same model with the charges cut off the graph: forces without the dq/dR term
    x = small_batch(dev)
    x[properties.R].requires_grad_()
    y = model.representation(A.PairwiseDistances()(x))
    y = model.output_modules[0](y)
    y[properties.partial_charges] = y[properties.partial_charges].detach()
    for m in list(model.output_modules)[1:4]:
        y = m(y)
    F_cut = -torch.autograd.grad(y["energy"].sum(), [x[properties.R]])[0]
    term = rel(F_cut, ref["forces"])
    print("electrostatics predicted charges: E %.3e F %.3e q %.3e; without dq/dR the forces are off by %.3e" % (eE, eF, eq, term))
    assert eE < TOL and eF < TOL and eq < TOL
    assert term > 100 * TOL                                                           # the dq/dR term is really there


def test_charges_without_a_consumer_still_carry_the_eval_guard(dev):
    rep = PaiNN(64, 2, GaussianRBF(20, 5.0), CosineCutoff(5.0))
    head = A.DipoleMoment(64, use_vector_representation=True, return_charges=True)
    model = M.NeuralNetworkPotential(rep, input_modules=[A.PairwiseDistances()],
                                     output_modules=[A.Atomwise(64, output_key="energy"), A.Forces(), head]).to(dev).eval()
    assert not head._charges_differentiable and M.classify_potential(model) == 2
    out = model(small_batch(dev))
    q = out["partial_charges"]
    assert q.requires_grad
    with pytest.raises(RuntimeError, match="eval"):
        q.sum().backward()


def test_aten_route_conditions_take_the_fallback(dev):
    (c, inp), v = case("E2", dev), EO.variant(GOLD, "E2", "k4")

    class Foreign(torch.nn.Module):
        def forward(self, d):
            return 1.0 / d

    def took_fallback(mod, x, strain=False):
        n0 = fallback.fallback_count()
        if strain:
            x = A.Strain()(x)
        mod(A.PairwiseDistances()(x))
        return fallback.fallback_count() > n0

    f64 = {k: (t.double() if torch.is_tensor(t) and t.is_floating_point() else t) for k, t in inp.items()}
    coul, ewald = coulomb_mirror("damped_cut", dev), ewald_mirror("E2", v, dev)
    assert not took_fallback(coul, fresh(inp)) and not took_fallback(ewald, fresh(inp))
    assert took_fallback(coul.train(), fresh(inp)) and took_fallback(ewald.train(), fresh(inp))                        # training mode
    coul.eval(), ewald.eval()
    assert took_fallback(coulomb_mirror("plain", dev).double(), f64) and took_fallback(ewald_mirror("E2", v, dev).double(), f64)   # float64
    foreign = A.EnergyCoulomb("eV", "Ang", Foreign(), "e", use_neighbors_lr=False).to(dev).eval()
    assert foreign._kind == -1 and took_fallback(foreign, fresh(inp))                                                     # a foreign potential
    screened = A.EnergyEwald(0.16, 4, "eV", "Ang", "e", use_neighbors_lr=False, screening_fn=CosineCutoff(3.0)).to(dev).eval()
    assert took_fallback(screened, fresh(inp))                                                                            # a foreign screening callable
    assert took_fallback(ewald, fresh(inp), strain=True) and not took_fallback(coul, fresh(inp), strain=True)             # a strained cell


def test_ewald_stress_goes_through_the_aten_route(dev):
    (c, inp), v = case("E2", dev), EO.variant(GOLD, "E2", "k4")
    model = schnet_model(ewald_mirror("E2", v, dev, lr=True), dev, strain=True, stress=True)
    out = model(model_inputs(inp, len(c["R"])))
    assert rel(out["e"], v["E"]) < TOL and rel(out["forces"], v["F"]) < TOL and bool(torch.isfinite(out["stress"]).all())


@pytest.mark.parametrize("which", ["coulomb", "ewald"])
def test_scripted_mirrors_equal_the_eager_ones(dev, which):
    if which == "coulomb":
        (c, inp), mod = case("C1", dev), coulomb_mirror("damped_cut", dev)
    else:
        (c, inp), mod = case("E2", dev), ewald_mirror("E2", EO.variant(GOLD, "E2", "k4_screened"), dev)
    scripted = torch.jit.script(mod)
    res = []
    for f in (mod, scripted):
        x = fresh(inp)
        x["_n_molecules"] = torch.tensor(int(c["n_mol"]))
        y = f(A.PairwiseDistances()(x))
        res.append((y["e"],) + torch.autograd.grad(y["e"].sum(), [x[properties.R], x[properties.partial_charges]]))
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_parameter_buffer_is_refreshed_in_place(dev):
    (c, inp) = case("C1", dev)
    mod = coulomb_mirror("damped_cut", dev)
    x = A.PairwiseDistances()(fresh(inp))
    e1 = mod(dict(x))["e"].clone()
    buf = mod._op_params
    mod.ke.mul_(2.0)
    e2 = mod(dict(x))["e"]
    assert mod._op_params is buf and torch.allclose(e2, 2.0 * e1, rtol=1e-6)
