"""GPU: the ZBL repulsion kernels (csrc/spk_zbl.hip) through every route -- the C ABI, ``torch.ops.spk_hip.zbl`` + autograd, the module mirror
inside a module-by-module model, the fused mode-4 / 5 routes of SchNet and PaiNN -- against the float64 fixture the reference's own code
produced (tests/golden/zbl_cases.npz, tests/make_zbl_golden.py).

Tolerance: the project's parity contract, 1e-5 relative in the max-norm, on E, F and W, with no extra margin; the
reference's own float32 gap on these cases is below a quarter of it (``gap_*`` in the fixture).  Every test prints what it measured.
The deployed runtime (``export_potential`` -> ``DeployedPotential``) is compared with the torch route on cases (b) and (d), virial included.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zbl_oracle as ZO  # noqa: E402

from schnetpack_amd import _lib, model as M, properties, synthetic as S  # noqa: E402
from schnetpack_amd._lib import fptr, iptr, stream  # noqa: E402
from schnetpack_amd.atomistic import Aggregation, Atomwise, Forces, PairwiseDistances, Strain, ZBLRepulsionEnergy  # noqa: E402
from schnetpack_amd.nn import CosineCutoff, GaussianRBF  # noqa: E402
from schnetpack_amd.representation import PaiNN, SchNet  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1.0e-5
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zbl_cases.npz"))
SORTED_SYMMETRIC = [t for t in ZO.CASES if not t.startswith("e_")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    return torch.device("cuda", 0)


def rel(x, ref):
    ref = np.asarray(ref, dtype=np.float64)
    x = x.detach().cpu().double().numpy() if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(x.reshape(ref.shape) - ref).max() / (scale if scale > 0 else 1.0))


_CASES = {}


def case(tag, dev):
    """Fixture case on the device (built once, never modified): arrays, float32 device inputs, the 12 parameters."""
    if tag not in _CASES:
        c = ZO.case_inputs(GOLD, tag)
        t = lambda k, dt: torch.tensor(c[k], dtype=dt, device=dev)
        inp = {properties.Z: t("Z", torch.long), properties.R: t("R", torch.float32), properties.cell: t("cell", torch.float32),
               properties.offsets: t("offsets", torch.float32), properties.idx_i: t("idx_i", torch.long), properties.idx_j: t("idx_j", torch.long),
               properties.idx_m: t("idx_m", torch.long), "_n_molecules": int(c["n_mol"])}
        prm = torch.tensor(ZO.case_params12(c), dtype=torch.float32, device=dev)
        _CASES[tag] = (c, inp, prm)
    return _CASES[tag]


def mirror_of(c, dev):
    cut = CosineCutoff(float(c["rc"])) if float(c["rc"]) > 0 else None
    mod = ZBLRepulsionEnergy(str(c["energy_unit"]), str(c["position_unit"]), "e_zbl", cutoff_fn=cut)
    mod.load_state_dict({k: torch.as_tensor(c[k], dtype=torch.float32) for k in ("ke", "a_pow", "a_div", "exponents", "coefficients")}, strict=False)
    return mod.to(dev).eval()


def check(tag, route, c, E, F, W=None):
    eE, eF = rel(E, c["E"]), rel(F, c["F"])
    eW = rel(W, c["W"]) if W is not None else 0.0
    print("zbl %-6s %-8s E %.3e F %.3e W %.3e" % (tag, route, eE, eF, eW))
    assert eE < TOL and eF < TOL and eW < TOL, (tag, route, eE, eF, eW)


# ----------------------------------------------------------------------------------------------------------------- C ABI
def c_abi(tag, dev):
    from schnetpack_amd import ops
    c, inp, prm = case(tag, dev)
    L = _lib.lib()
    R, off, Z, idx_m, n_mol = inp[properties.R], inp[properties.offsets], inp[properties.Z], inp[properties.idx_m], int(c["n_mol"])
    N = R.shape[0]
    r = torch.ops.spk_hip.pairwise(R, inp[properties.idx_i], inp[properties.idx_j], off)
    plan = ops.EdgePlan(inp[properties.idx_i], inp[properties.idx_j], N, r)
    ws = torch.empty(int(L.spk_zbl_workspace_bytes(plan.graph(), n_mol)), dtype=torch.uint8, device=dev)
    E, Ea = torch.full((n_mol,), 7.0, device=dev), torch.full((N,), 7.0, device=dev)
    _lib.check(L.spk_zbl_fwd_f32(fptr(r), iptr(Z), plan.graph(), iptr(idx_m), n_mol, fptr(prm), fptr(E), fptr(Ea), ctypes.c_void_p(ws.data_ptr()), stream()))
    gr = torch.empty_like(r)
    _lib.check(L.spk_zbl_bwd_f32(fptr(torch.ones(n_mol, device=dev)), fptr(r), iptr(Z), plan.graph(), iptr(idx_m), n_mol, fptr(prm), fptr(gr), stream()))
    return c, inp, prm, plan, ws, r, E, Ea, gr


@pytest.mark.parametrize("tag", ZO.CASES)
def test_c_abi_forward_and_backward(dev, tag):
    c, inp, prm, plan, ws, r, E, Ea, gr = c_abi(tag, dev)
    L, N, n_mol = _lib.lib(), inp[properties.R].shape[0], int(c["n_mol"])
    gR = torch.empty(N, 3, device=dev)
    _lib.check(L.spk_pairwise_bwd_graph_f32(fptr(gr), plan.graph(), fptr(gR), stream()))
    W = torch.empty(n_mol, 3, 3, device=dev)
    vws = torch.empty(int(L.spk_edge_virial_workspace_bytes(plan.graph(), n_mol, 0)), dtype=torch.uint8, device=dev)
    _lib.check(L.spk_edge_virial_f32(fptr(gr), fptr(inp[properties.R]), fptr(inp[properties.offsets]), plan.graph(), iptr(inp[properties.idx_m]), n_mol,
                                     fptr(W), None, ctypes.c_void_p(vws.data_ptr()), stream()))
    assert rel(Ea, c["E_atom"]) < TOL
    check(tag, "c-abi", c, E, -gR, W)


@pytest.mark.parametrize("tag", SORTED_SYMMETRIC)
def test_c_abi_fused_forces_add_in_place_and_are_bit_reproducible(dev, tag):
    c, inp, prm, plan, ws, r, E, Ea, gr = c_abi(tag, dev)
    assert plan.sorted and plan.symmetric
    L, N, n_mol = _lib.lib(), inp[properties.R].shape[0], int(c["n_mol"])
    outs = []
    for _ in range(2):
        F, W, Ez = torch.full((N, 3), 0.5, device=dev), torch.full((n_mol, 3, 3), -0.25, device=dev), torch.full((n_mol,), 7.0, device=dev)
        _lib.check(L.spk_zbl_forces_f32(fptr(inp[properties.R]), fptr(inp[properties.offsets]), iptr(inp[properties.Z]), plan.graph(),
                                        iptr(inp[properties.idx_m]), n_mol, fptr(prm), fptr(Ez), fptr(F), fptr(W), ctypes.c_void_p(ws.data_ptr()), stream()))
        outs.append((Ez, F, W))
    assert all(torch.equal(a, b) for a, b in zip(*outs))                          # two calls on the same list: the same bits
    Ez, F, W = outs[0]
    check(tag, "fused", c, Ez, F - 0.5, W + 0.25)
    deg = np.bincount(c["idx_i"], minlength=N)
    if (deg == 0).any():                                                          # an atom without pairs: E_atom = 0, F untouched
        lone = torch.tensor(np.nonzero(deg == 0)[0], device=dev)
        assert bool((F[lone] == 0.5).all()) and bool((Ea[lone] == 0).all())
    if tag == "b":
        assert float(Ez[-1]) == 0.0 and float(E[-1]) == 0.0 and bool((W[-1] == -0.25).all())       # the molecule without atoms
    # without W: the same energies and forces
    F2, E2 = torch.full((N, 3), 0.5, device=dev), torch.empty(n_mol, device=dev)
    _lib.check(L.spk_zbl_forces_f32(fptr(inp[properties.R]), fptr(inp[properties.offsets]), iptr(inp[properties.Z]), plan.graph(), iptr(inp[properties.idx_m]),
                                    n_mol, fptr(prm), fptr(E2), fptr(F2), None, ctypes.c_void_p(ws.data_ptr()), stream()))
    assert torch.equal(E2, Ez) and torch.equal(F2, F)


def test_c_abi_refuses_the_row_pass_on_a_half_list(dev):
    c, inp, prm, plan, ws, r, E, Ea, gr = c_abi("e_half", dev)
    N, n_mol = inp[properties.R].shape[0], int(c["n_mol"])
    F, Ez = torch.zeros(N, 3, device=dev), torch.empty(n_mol, device=dev)
    rc = _lib.lib().spk_zbl_forces_f32(fptr(inp[properties.R]), None, iptr(inp[properties.Z]), plan.graph(), iptr(inp[properties.idx_m]), n_mol, fptr(prm),
                                       fptr(Ez), fptr(F), None, ctypes.c_void_p(ws.data_ptr()), stream())
    assert rc != 0 and b"spk_zbl_bwd_f32" in _lib.lib().spk_last_error() and bool((F == 0).all())


def test_skin_pairs_pad_atoms_and_atomic_numbers_out_of_range(dev):
    c, inp, prm = case("f", dev)
    R, off, ii, jj, idx_m, n_mol = inp[properties.R], inp[properties.offsets], inp[properties.idx_i], inp[properties.idx_j], inp[properties.idx_m], int(c["n_mol"])
    r = torch.ops.spk_hip.pairwise(R, ii, jj, off)
    d = r.norm(dim=1)
    skin = d >= float(c["rc"])
    assert int(skin.sum()) >= 2
    gr = torch.ops.spk_hip.zbl_backward(torch.ones(n_mol, device=dev), r, inp[properties.Z], ii, jj, idx_m, n_mol, prm)
    assert bool((gr[skin] == 0).all()) and bool((gr[~skin] != 0).any())                          # skin pairs: exact zeros
    # the results on the skin list equal those on the list built at the radius bit for bit only if the skin adds exact zeros to each row
    cb, inb, _ = case("b", dev)
    Eb = torch.ops.spk_hip.zbl(torch.ops.spk_hip.pairwise(inb[properties.R], inb[properties.idx_i], inb[properties.idx_j], inb[properties.offsets]),
                               inb[properties.Z], inb[properties.idx_i], inb[properties.idx_j], idx_m, n_mol, prm)[0]
    Ef = torch.ops.spk_hip.zbl(r, inp[properties.Z], ii, jj, idx_m, n_mol, prm)[0]
    assert rel(Ef, Eb.cpu().double().numpy()) < 1e-6
    # Z = 0 (pad atoms): exact zeros in its own row and in its neighbours' pairs with it
    Z0 = inp[properties.Z].clone()
    Z0[8:] = 0                                                                                   # the whole last molecule
    F, W = torch.zeros_like(R), torch.zeros(n_mol, 3, 3, device=dev)
    E0 = torch.ops.spk_hip.zbl_forces(R, off, Z0, ii, jj, idx_m, n_mol, prm, F, W)
    assert float(E0[3]) == 0.0 and bool((F[8:] == 0).all()) and bool((W[3] == 0).all()) and float(E0[2]) != 0.0
    # Z outside [0, 128): NaN in that atom's outputs (and in its partners'), finite elsewhere, no fault
    Zb = inp[properties.Z].clone()
    Zb[9], Zb[10] = 200, -3
    F = torch.zeros_like(R)
    Ebad = torch.ops.spk_hip.zbl_forces(R, off, Zb, ii, jj, idx_m, n_mol, prm, F, None)
    Ea = torch.ops.spk_hip.zbl(r, Zb, ii, jj, idx_m, n_mol, prm)[1]
    torch.cuda.synchronize()
    assert bool(torch.isnan(F[9]).all()) and bool(torch.isnan(F[10]).all()) and bool(torch.isnan(Ea[9])) and bool(torch.isnan(Ebad[3]))
    assert bool(torch.isfinite(F[:8]).all()) and bool(torch.isfinite(Ebad[:3]).all()) and bool(torch.isfinite(Ea[:8]).all())


def test_row_pass_adds_exact_zeros_for_skin_pairs_and_coincident_pad_atoms(dev):
    """Rows made only of pairs that must not count: atoms 0 / 1 are 5.5 A apart (beyond the 5 A radius), atoms 2 / 3 are pad atoms (Z = 0) on the
    same point (d = 0).  The fused row pass must leave the prefilled F and W bit for bit as they are and return E = 0; so must the edge route."""
    c, inp, prm = case("b", dev)
    R = torch.tensor([[0.0, 0.0, 0.0], [3.3, 4.4, 0.0], [9.0, 9.0, 9.0], [9.0, 9.0, 9.0]], device=dev)
    Z = torch.tensor([6, 8, 0, 0], device=dev)
    ii, jj = torch.tensor([0, 1, 2, 3], device=dev), torch.tensor([1, 0, 3, 2], device=dev)
    idx_m = torch.tensor([0, 0, 1, 1], device=dev)
    F, W = torch.full((4, 3), 0.5, device=dev), torch.full((2, 3, 3), -0.25, device=dev)
    E = torch.ops.spk_hip.zbl_forces(R, None, Z, ii, jj, idx_m, 2, prm, F, W)
    assert bool((E == 0).all()) and bool((F == 0.5).all()) and bool((W == -0.25).all())
    r = torch.ops.spk_hip.pairwise(R, ii, jj, None)
    E2, Ea = torch.ops.spk_hip.zbl(r, Z, ii, jj, idx_m, 2, prm)
    gr = torch.ops.spk_hip.zbl_backward(torch.ones(2, device=dev), r, Z, ii, jj, idx_m, 2, prm)
    assert bool((E2 == 0).all()) and bool((Ea == 0).all()) and bool((gr == 0).all())


# ----------------------------------------------------------------------------------------------------------------- operator + autograd
@pytest.mark.parametrize("tag", ZO.CASES)
def test_operator_with_autograd(dev, tag):
    c, inp, prm = case(tag, dev)
    n_mol = int(c["n_mol"])
    R = inp[properties.R].clone().requires_grad_()
    off = inp[properties.offsets].clone().requires_grad_()
    r = torch.ops.spk_hip.pairwise(R, inp[properties.idx_i], inp[properties.idx_j], off)
    E, Ea = torch.ops.spk_hip.zbl(r, inp[properties.Z], inp[properties.idx_i], inp[properties.idx_j], inp[properties.idx_m], n_mol, prm)
    gR, gr = torch.autograd.grad(E.sum(), [R, r])
    assert E.shape == (n_mol,) and rel(Ea, c["E_atom"]) < TOL
    W = torch.zeros(n_mol, 3, 3, device=dev).index_add_(0, inp[properties.idx_m][inp[properties.idx_i]], gr[:, :, None] * r.detach()[:, None, :])
    check(tag, "op", c, E, -gR, W)
    # a second-order request names the way out
    E2 = torch.ops.spk_hip.zbl(r, inp[properties.Z], inp[properties.idx_i], inp[properties.idx_j], inp[properties.idx_m], n_mol, prm)[0]
    with pytest.raises(RuntimeError, match="training mode"):
        torch.autograd.grad(E2.sum(), R, create_graph=True)


# ----------------------------------------------------------------------------------------------------------------- models
_MODELS = {}


def zbl_models(kind, tag, dev):
    """(fused mode-5 model, the same modules run module by module, the same representation and head without the ZBL term)."""
    c = case(tag, dev)[0]
    rep_key = (kind, round(float(c["rc"]), 3))
    if (kind, tag) not in _MODELS:
        if rep_key not in _MODELS:
            torch.manual_seed(5)
            rc_rep = max(float(c["rc"]), 5.0) * 1.31            # every delivered pair (skin list included) inside the representation's cutoff
            rep = (SchNet if kind == "schnet" else PaiNN)(64, 1, GaussianRBF(8, rc_rep), CosineCutoff(rc_rep))
            _MODELS[rep_key] = (rep, Atomwise(n_in=64, output_key="e_nn"))
        rep, head = _MODELS[rep_key]

        def build(stress):
            outs = [head, mirror_of(c, dev), Aggregation(["e_nn", "e_zbl"], properties.energy), Forces(calc_forces=True, calc_stress=stress)]
            return M.NeuralNetworkPotential(rep, input_modules=([Strain()] if stress else []) + [PairwiseDistances()], output_modules=outs).to(dev).eval()
        fused4, fused5, slow = build(False), build(True), build(True)
        assert M.classify_potential(fused4) == 4 and M.classify_potential(fused5) == 5
        slow._potential_zbl = False                                                               # module by module
        plain = M.NeuralNetworkPotential(rep, input_modules=[Strain(), PairwiseDistances()],
                                         output_modules=[head, Forces(calc_forces=True, calc_stress=True, energy_key="e_nn")]).to(dev).eval()
        assert M.classify_potential(plain) == 3
        _MODELS[(kind, tag)] = (fused4, fused5, slow, plain)
    return _MODELS[(kind, tag)]


def run(model, inp):
    out = model({k: (v.clone() if torch.is_tensor(v) else v) for k, v in inp.items()})
    return {k: v.detach() for k, v in out.items()}


@pytest.mark.parametrize("kind", ["schnet", "painn"])
@pytest.mark.parametrize("tag", ZO.CASES)
def test_fused_routes_and_module_by_module_route_of_a_model(dev, kind, tag):
    c, inp, prm = case(tag, dev)
    fused4, fused5, slow, plain = zbl_models(kind, tag, dev)
    o4, o5, os_, op = run(fused4, inp), run(fused5, inp), run(slow, inp), run(plain, inp)
    vol = torch.det(inp[properties.cell])[:, None, None]
    for route, o in (("mode-5", o5), ("modules", os_)):
        # the ZBL share of the model's outputs: what the term adds to the same representation and head without it
        check(tag, kind[:2] + "-" + route, c, o[properties.energy] - op["e_nn"], o[properties.forces] - op[properties.forces],
              (o[properties.stress] - op[properties.stress]) * vol)
    check(tag, kind[:2] + "-mode-4", c, o4[properties.energy] - op["e_nn"], o4[properties.forces] - op[properties.forces])
    # the fused route equals the module-by-module route on the same model
    for k in (properties.energy, "e_nn", properties.forces, properties.stress):
        e = rel(o5[k], os_[k].cpu().double().numpy())
        print("zbl %-6s %s fused against modules %-8s %.3e" % (tag, kind, k, e))
        assert e < TOL, (k, e)
    assert rel(o4[properties.forces], o5[properties.forces].cpu().double().numpy()) < TOL


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_graphed_force_call_replay_equals_eager(dev, kind):
    from schnetpack_amd.forcecall import GraphedForceCall
    c, inp, prm = case("b", dev)
    fused4 = zbl_models(kind, "b", dev)[0]
    batch = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in inp.items() if k != properties.cell}
    call = GraphedForceCall(fused4)
    call(batch)
    assert call.graph is not None
    moved = dict(batch)
    moved[properties.R] = batch[properties.R] + 0.02 * torch.randn(batch[properties.R].shape, generator=torch.Generator().manual_seed(1)).to(dev)
    res = {k: v.clone() for k, v in call(moved).items()}
    assert call.n_captures == 1
    eager = run(fused4, moved)
    for k in ("energy", "forces"):
        e = rel(res[k], eager[k].cpu().double().numpy())
        print("zbl graph replay against eager %s %-7s %.3e" % (kind, k, e))
        assert e < 1e-6                                                                           # (float atomics of the representation: summation order)
    assert not torch.equal(res["forces"], run(fused4, batch)["forces"])                         # the replay saw the new positions


def test_nvt_simulation_with_a_zbl_model(dev):
    """Five NVT steps (global Nose-Hoover chain) of a PaiNN + ZBL model on three molecules: the run as graph replays equals the eager run
    bit for bit and the total energy is the potential plus the kinetic energy of the kinetic kernel -- what tests/test_gpu_md_thermostat.py
    checks of the model without the term."""
    from schnetpack_amd import md as MD
    systems = []
    for Z, R in ((S.ASPIRIN_Z, S.ASPIRIN_R), (S.ETHANOL_Z, S.ETHANOL_R), (S.ETHANOL_Z[:6], S.ETHANOL_R[:6])):
        R = np.asarray(R, dtype=np.float64)
        ii, jj = S.neighbor_pairs_open(R, 5.0)
        systems.append({"Z": list(Z), "R": R, "idx_i": ii, "idx_j": jj})
    b, sizes = S.collate(systems), [21, 9, 6]
    torch.manual_seed(11)
    rep = PaiNN(128, 1, GaussianRBF(20, 5.0), CosineCutoff(5.0))
    outs = [Atomwise(n_in=128, output_key="e_nn"), ZBLRepulsionEnergy("eV", "Ang", "e_zbl", cutoff_fn=CosineCutoff(4.0)),
            Aggregation(["e_nn", "e_zbl"], properties.energy), Forces()]
    model = M.NeuralNetworkPotential(rep, input_modules=[PairwiseDistances()], output_modules=outs).to(dev).eval()
    assert M.classify_potential(model) == 4
    masses = torch.where(b["Z"] == 1, 1.008, torch.where(b["Z"] == 6, 12.011, 15.999))
    sims = []
    for use_graph in (True, False):
        inp = M.batch_to_inputs(b, dev)
        inp["_n_atoms"] = torch.tensor(sizes, device=dev)
        sim = MD.NVTSimulation(model, inp, masses.to(dev), 0.02, cutoff=5.0, thermostat=MD.NHCThermostat(0.05, 0.1, fs=1.0, kb=1.0), cutoff_shell=0.3,
                               use_graph=use_graph)
        p0 = 0.3 * torch.randn(b["R"].shape, generator=torch.Generator().manual_seed(0)) * masses[:, None].sqrt()
        sim.state.momenta.copy_(p0.to(dev).unsqueeze(0))
        sim.step(5)
        sims.append(sim)
    sim_g, sim_e = sims
    assert sim_g.graph is not None and sim_e.graph is None and sim_g.step_count == 5
    assert torch.equal(sim_g.state.positions, sim_e.state.positions) and torch.equal(sim_g.state.momenta, sim_e.state.momenta)
    assert bool(torch.isfinite(sim_g.state.momenta).all())
    idx_m = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    ke = 0.5 * torch.zeros(3, dtype=torch.float64).index_add_(0, idx_m, (sim_g.state.momenta[0].cpu().double() ** 2).sum(1) / masses.double())
    assert rel(sim_g.kinetic_energy(), ke.numpy()) < 1e-6
    assert abs(sim_g.total_energy() - (float(sim_g.energy.sum()) + float(ke.sum()))) < 1e-4 * float(ke.sum())
    # the repulsion is part of the potential energy the simulation reports
    out = run(model, {**M.batch_to_inputs(b, dev), properties.R: sim_g.state.positions[0].clone()})
    assert rel(sim_g.energy, out[properties.energy].cpu().double().numpy()) < 1e-5 and float((out[properties.energy] - out["e_nn"]).abs().min()) > 0


# ----------------------------------------------------------------------------------------------------------------- deployed runtime
@pytest.mark.parametrize("kind", ["schnet", "painn"])
@pytest.mark.parametrize("tag", ["b", "d"])
def test_deployed_potential_of_a_zbl_model_equals_the_torch_route(dev, kind, tag):
    from schnetpack_amd import deploy
    c, inp, prm = case(tag, dev)
    fused4, fused5, slow, plain = zbl_models(kind, tag, dev)
    ref = run(fused5, inp)
    vol = torch.det(inp[properties.cell])[:, None, None]
    pot = deploy.DeployedPotential(deploy.export_potential(fused5))
    n_mol = int(c["n_mol"])
    args = (c["Z"], c["R"], c["idx_i"], c["idx_j"], c["offsets"], c["idx_m"], n_mol)
    E, F, W = pot.compute(*args, virial=True)
    E1, F1 = pot.compute(*args)
    assert rel(E1, E) < TOL and rel(F1, F) < TOL                # (the entry point without the virial; SchNet sums with float atomics: not bit for bit)
    for name, got, want in (("E", E, ref[properties.energy]), ("F", F, ref[properties.forces]), ("W", W, ref[properties.stress] * vol)):
        e = rel(got, want.cpu().double().numpy())
        print("zbl %-2s %s deployed against the torch route %s %.3e" % (tag, kind, name, e))
        assert e < TOL, (name, e)
    # the term is in there: the file of the same model without it gives other forces
    Ep, Fp = deploy.DeployedPotential(deploy.export_potential(plain)).compute(*args)
    assert rel(F - Fp, c["F"]) < TOL and rel(E - Ep, c["E"]) < TOL
    if tag == "b":
        # the list the runtime builds itself (at the representation's cutoff: it holds pairs beyond the ZBL radius) against the same list handed over
        rc = pot.cutoff
        d = np.linalg.norm(c["R"][None] - c["R"][:, None], axis=2)
        ii, jj = np.nonzero((d < rc) & ~np.eye(len(d), dtype=bool))
        assert (d[ii, jj] >= float(c["rc"])).any()
        n_mol = 4                                                  # (the molecules that have atoms: the runtime's list builder wants a cell per system)
        cell, pbc = c["cell"][:n_mol], np.zeros((n_mol, 3), dtype=np.uint8)
        Ec, Fc, Wc = pot.compute_cell(c["Z"], c["R"], cell, pbc, idx_m=c["idx_m"], n_mol=n_mol, virial=True)
        El, Fl, Wl = pot.compute(c["Z"], c["R"], ii, jj, None, c["idx_m"], n_mol, virial=True)
        assert pot.last_stats["pairs"] == len(ii)
        for name, a, b in (("E", Ec, El), ("F", Fc, Fl), ("W", Wc, Wl)):
            e = rel(a, b)
            print("zbl b  %s deployed: own list against the list handed over %s %.3e" % (kind, name, e))
            assert e < TOL
        Ec2, Fc2 = pot.compute_cell(c["Z"], c["R"], cell, pbc, idx_m=c["idx_m"], n_mol=n_mol)
        assert rel(Fc2, Fc) < TOL and rel(Ec2, Ec) < TOL
    pot.close()
