"""GPU: the classical NVT thermostats (csrc/spk_md_thermo.hip, ``schnetpack_amd.md``) against the reference's fixture
(tests/golden/md_thermostat.npz) and, for shapes the fixture does not hold, against tests/md_thermostat_oracle.py.

Tolerances (``md_thermostat_oracle.allowed_error``): 4 x the reference's own float32-versus-float64 gap on the same case, floor
4 float32 ulp of the quantity's magnitude; for oracle-only shapes the gap is that of the oracle evaluated in float32 (the same
arithmetic).  ``ke2`` against float64: the summation bound ``ke2_bound``.  Every test prints what it measured.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_npz, rel_err
from oracle import md_oracle as MDO
from oracle import spk_oracle as O
from schnetpack_amd import synthetic as S

import md_thermostat_oracle as TO

pytestmark = pytest.mark.gpu
APPS = (1, 6)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def g():
    return load_npz("md_thermostat.npz")


def T(x):
    return torch.from_numpy(np.asarray(x))


def layout(sizes):
    n = torch.tensor(sizes, dtype=torch.long)
    return torch.repeat_interleave(torch.arange(len(sizes)), n), n


def thermal(n_rep, n_atoms, seed):
    gen = torch.Generator().manual_seed(seed)
    m = (torch.rand(n_atoms, generator=gen) * 15 + 1).float()
    p = (torch.randn(n_rep, n_atoms, 3, generator=gen) * m[None, :, None].sqrt() * 1.5).float()
    return p, m


def device_ke2(dev, p, m, idx_m, n_mol, err=None):
    from schnetpack_amd.md import _ThermostatHip as H
    n_rep, N = p.shape[0], p.shape[1]
    ke2 = torch.full((n_rep * n_mol,), float("nan"), device=dev)
    ws = H.workspace(n_rep, N, n_mol, dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev) if err is None else err
    H.kinetic(p.to(dev).contiguous(), m.to(dev), idx_m.to(dev), n_mol, ke2, err, ws)
    return ke2.view(n_rep, n_mol), err


# ----------------------------------------------------------------------------- kinetic reduction
SIZES = [1, 2, 63, 64, 65, 200]
KIN_CASES = {"mixed": (1, SIZES), "empties": (1, [0, 0] + SIZES[:3] + [0] + SIZES[3:] + [0, 0]), "600x3": (1, [3] * 600), "one5000": (1, [5000]),
             "2x3": (2, [7, 64, 130]), "fixture": (2, [2, 5, 9])}


@pytest.mark.parametrize("case", sorted(KIN_CASES))
def test_kinetic_matches_float64_within_summation_roundoff_and_is_bit_reproducible(dev, case):
    n_rep, sizes = KIN_CASES[case]
    idx_m, n = layout(sizes)
    p, m = thermal(n_rep, int(n.sum()), 11)
    got, err = device_ke2(dev, p, m, idx_m, len(sizes))
    again, _ = device_ke2(dev, p, m, idx_m, len(sizes))
    assert torch.equal(got, again) and int(err.item()) == 0
    ref = TO.kinetic_energy2(p.double(), m.double(), idx_m, len(sizes))
    bound = TO.ke2_bound(p, m, idx_m, n)
    diff = (got.cpu().double() - ref).abs()
    print("ke2 %s: worst error / bound %.3f" % (case, float((diff / bound.clamp_min(1e-300)).max())))
    assert bool((diff <= bound).all())
    assert bool((got.cpu()[:, n == 0] == 0).all())          # exactly 0, not merely small


def test_kinetic_reports_a_malformed_index_without_using_it(dev):
    """Descending and out-of-range molecule indices: err bits 1 / 2, finite or untouched outputs, no fault."""
    p, m = thermal(1, 6, 5)
    for idx, bit in (([2, 2, 1, 1, 0, 0], 1), ([0, 0, 1, 7, 7, 7], 2), ([0, 0, -3, 1, 2, 2], 2)):
        got, err = device_ke2(dev, p, m, torch.tensor(idx), 3)
        assert int(err.item()) & bit, (idx, int(err.item()))
        from schnetpack_amd.md import _ThermostatHip as H
        pd = p.to(dev).contiguous()
        e2 = torch.zeros(1, dtype=torch.int32, device=dev)
        H.scale_molecules(pd, torch.full((3,), 2.0, device=dev), torch.tensor(idx, device=dev), 3, e2)
        ok = torch.tensor([0 <= i < 3 for i in idx])
        assert torch.equal(pd.cpu()[0, ok], 2 * p[0, ok]) and torch.equal(pd.cpu()[0, ~ok], p[0, ~ok])
        assert (int(e2.item()) & 2) == (2 if bool((~ok).any()) else 0)


# ----------------------------------------------------------------------------- Nose-Hoover chains
def nhc_for(g, tag, dev):
    from schnetpack_amd import md as MD
    L, ms, order, massive = (int(x) for x in g["nhc_params"][list(g["nhc_cases"]).index(tag)])
    return MD.NHCThermostat(float(g["temperature_bath"]), float(g["tau_fs"]), L, bool(massive), ms, order)


def fixture_state(g, dev):
    from schnetpack_amd import md as MD
    return MD.MDState(T(g["q"]).float().to(dev), T(g["p"]).float().to(dev).contiguous(), T(g["masses"]).float().reshape(1, -1, 1).to(dev))


def nhc_tags():
    import make_md_thermostat_golden as G
    return [c[0] for c in G.NHC_CASES]


@pytest.mark.parametrize("tag", nhc_tags())
def test_nhc_matches_the_reference_fixture(dev, g, tag):
    """1 and 6 consecutive applications on the fixture system: scale, chain velocities / forces and momenta."""
    import types
    state = fixture_state(g, dev)
    th = nhc_for(g, tag, dev).init(types.SimpleNamespace(time_step=float(g["dt"])), T(g["idx_m"]), T(g["n_atoms"]))
    for k in range(1, 7):
        before = state.momenta.clone()
        th.apply(state)
        if k in APPS:
            sd = th.state_dict()
            scale = (state.momenta / before) if th.massive else th.scaling_factor
            for name, got in (("scale", scale), ("v", sd["velocities"]), ("f", sd["forces"]), ("p", state.momenta)):
                r64, r32 = T(g["nhc_%s_f64_%s_%d" % (tag, name, k)]), T(g["nhc_%s_f32_%s_%d" % (tag, name, k)])
                e, tol = float((got.cpu().double().reshape(r64.shape) - r64).abs().max()), TO.allowed_error(r64, r32)
                print("nhc %s %s after %d: error %.3e allowed %.3e (reference float32 gap %.3e)" % (tag, name, k, e, tol, float((r32 - r64).abs().max())))
                assert e <= tol, (name, k, e, tol)
    assert int(th._err.item()) == 0


def oracle_nhc(p, m, idx_m, n, th, n_apps, dtype):
    """The oracle in ``dtype`` on the float32 inputs: (p, v, f, scale) after ``n_apps`` applications."""
    L = th.chain_length
    p, m = p.to(dtype), m.to(dtype)
    steps = torch.tensor(th.sub_steps, dtype=dtype)
    v = torch.zeros(tuple(p.shape) + (L,), dtype=dtype) if th.massive else torch.zeros(p.shape[0], len(n), L, dtype=dtype)
    f, s = torch.zeros_like(v), None
    for _ in range(n_apps):
        if th.massive:
            p = TO.nhc_apply_massive(p, m, th.kb_temperature, th.frequency, v, f, steps, th.multi_step)
        else:
            p, s = TO.nhc_apply_global(p, m, idx_m, n, th.kb_temperature, th.frequency, v, f, steps, th.multi_step)
    return p, v, f, s


@pytest.mark.parametrize("sizes,n_rep", [([0, 3, 0, 0, 65, 1, 0], 2), ([4] * 70, 1)])
def test_nhc_global_leaves_empty_molecules_alone(dev, sizes, n_rep):
    """Empty molecules leading, interior and trailing: their chains and scale stay (0, 1), nothing is non-finite; the others follow
    the oracle.  70 molecules: more chains than one 64-thread block."""
    import types
    from schnetpack_amd import md as MD
    idx_m, n = layout(sizes)
    p, m = thermal(n_rep, int(n.sum()), 3)
    th = MD.NHCThermostat(2.0, 0.1, fs=1.0, kb=1.0).init(types.SimpleNamespace(time_step=0.02), idx_m, n)
    state = MD.MDState(p.to(dev), p.to(dev).contiguous(), m.to(dev))
    for _ in range(3):
        th.apply(state)
    sd = {k: t.cpu() for k, t in th.state_dict().items()}
    empty, scale = n == 0, th.scaling_factor.cpu()
    assert all(bool(torch.isfinite(t).all()) for t in (sd["velocities"], sd["forces"], state.momenta, scale))
    assert bool((sd["velocities"][:, empty] == 0).all()) and bool((sd["forces"][:, empty] == 0).all()) and bool((scale[:, empty] == 1).all())
    r64, r32 = oracle_nhc(p, m, idx_m, n, th, 3, torch.float64), oracle_nhc(p, m, idx_m, n, th, 3, torch.float32)
    for name, got, a, b in (("p", state.momenta, r64[0], r32[0]), ("v", sd["velocities"].squeeze(2), r64[1], r32[1]), ("scale", th.scaling_factor, r64[3], r32[3])):
        e, tol = float((got.cpu().double() - a).abs().max()), TO.allowed_error(a, b)
        print("nhc empties %s: error %.3e allowed %.3e" % (name, e, tol))
        assert e <= tol, (name, e, tol)


@pytest.mark.parametrize("n_atoms", [1, 85, 1367])
def test_nhc_massive_sizes_that_are_no_multiple_of_the_workgroup(dev, n_atoms):
    import types
    from schnetpack_amd import md as MD
    p, m = thermal(2, n_atoms, 9)
    th = MD.NHCThermostat(2.0, 0.1, chain_length=3, massive=True, fs=1.0, kb=1.0).init(types.SimpleNamespace(time_step=0.02))
    state = MD.MDState(p.to(dev), p.to(dev).contiguous(), m.to(dev))
    for _ in range(2):
        th.apply(state)
    sd = th.state_dict()
    assert sd["velocities"].shape == (2, n_atoms, 3, 3)
    r64, r32 = oracle_nhc(p, m, None, None, th, 2, torch.float64), oracle_nhc(p, m, None, None, th, 2, torch.float32)
    for name, got, a, b in (("p", state.momenta, r64[0], r32[0]), ("v", sd["velocities"], r64[1], r32[1]), ("f", sd["forces"], r64[2], r32[2])):
        e, tol = float((got.cpu().double() - a).abs().max()), TO.allowed_error(a, b)
        print("nhc massive N=%d %s: error %.3e allowed %.3e" % (n_atoms, name, e, tol))
        assert e <= tol, (name, e, tol)


# ----------------------------------------------------------------------------- Berendsen, Langevin
def test_berendsen_matches_the_fixture_and_leaves_a_molecule_at_rest_alone(dev, g):
    import types
    from schnetpack_amd import md as MD
    state = fixture_state(g, dev)
    th = MD.BerendsenThermostat(float(g["temperature_bath"]), float(g["tau_fs"])).init(types.SimpleNamespace(time_step=float(g["dt"])), T(g["idx_m"]), T(g["n_atoms"]))
    for k in range(1, 7):
        th.apply(state)
        if k in (1, 2, 6):
            r64, r32 = T(g["ber_p_%d" % k]), T(g["ber_f32_p_%d" % k])
            e, tol = float((state.momenta.cpu().double() - r64).abs().max()), TO.allowed_error(r64, r32)
            print("berendsen after %d: error %.3e allowed %.3e" % (k, e, tol))
            assert e <= tol
    p = torch.zeros(1, 5, 3)
    p[0, 3:] = 1.0
    st = MD.MDState(p.to(dev), p.to(dev).contiguous(), torch.ones(5, device=dev))
    th.init(types.SimpleNamespace(time_step=1e-3), torch.tensor([0, 0, 0, 2, 2]), torch.tensor([3, 0, 2])).apply(st)
    out = st.momenta.cpu()
    assert bool(torch.isfinite(out).all()) and torch.equal(out[0, :3], p[0, :3]) and not torch.equal(out[0, 3:], p[0, 3:])


def test_langevin_is_the_one_bead_pile_kernel_and_matches_the_fixture(dev, g):
    import types
    from schnetpack_amd import md as MD
    dt, tau_fs, T0, seed = float(g["dt"]), float(g["tau_fs"]), float(g["temperature_bath"]), int(g["seed"])
    th = MD.LangevinThermostat(T0, tau_fs, seed=seed).init(types.SimpleNamespace(time_step=dt))
    state = fixture_state(g, dev)
    p0 = state.momenta.clone()
    th.apply(state, 0, 0)
    # The reference is handed the noise as float64 numbers; the kernel GENERATES it (Box-Muller: logf, sincosf in float32), an
    # error the reference's float32 gap does not contain.  This is spk_md_pile_f32 bit for bit (below), so its established bound
    # applies (tests/test_md_reference.py::pile_tolerance): 2e-5 |ref| + 2e-5 max|ref|.  The 4 x gap figure is printed.
    r64, r32 = T(g["lan_f64_p_out"]), T(g["lan_f32_p_out"])
    diff = (state.momenta.cpu().double() - r64).abs()
    print("langevin: error %.3e of max|ref| (4 x reference float32 gap: %.3e, kernel bound 2e-5)" % (float(diff.max() / r64.abs().max()), TO.allowed_error(r64, r32) / float(r64.abs().max())))
    assert bool((diff <= 2e-5 * r64.abs() + 2e-5 * float(r64.abs().max())).all())
    # bit for bit what spk_md_pile_f32 gives at one bead for the same (seed, step, which), also with the step on the device
    pile = MD.PILELocalThermostat(T0, tau_fs, seed=seed).init(MD.RingPolymer(dt, 1, T0, omega=7.0))
    for step, which in ((0, 0), (3, 1)):
        st = MD.MDState(p0, p0.clone(), state.masses)
        th.apply(st, step, which)
        flat = MD.MDState(p0, p0.reshape(1, -1, 3).clone(), state.masses.reshape(-1).repeat(2))
        want = pile.apply(flat, step, which)
        assert torch.equal(st.momenta.reshape(1, -1, 3), want)
        st2 = MD.MDState(p0, p0.clone(), state.masses)
        th.apply(st2, 0, which, torch.full((1,), step, dtype=torch.int64, device=dev))
        assert torch.equal(st2.momenta, st.momenta)


# ----------------------------------------------------------------------------- argument checks
def test_argument_checks(dev):
    from schnetpack_amd import _lib
    from schnetpack_amd._lib import SpkHipError, fptr, iptr, lib, stream
    L = lib()
    f = torch.ones(12, device=dev)
    n1 = torch.tensor([1], device=dev)
    i0 = torch.zeros(1, dtype=torch.long, device=dev)
    ws = torch.zeros(1024, dtype=torch.int32, device=dev)
    steps = (ctypes.c_float * 3)(0.01, -0.01, 0.01)
    assert L.spk_md_kinetic_workspace_bytes(-1, 1, 1) == -1 and L.spk_md_kinetic_workspace_bytes(1, 1, 1) > 0

    def bad(rc, what):
        assert rc != 0
        with pytest.raises(SpkHipError, match=what):
            _lib.check(rc)
    bad(L.spk_md_kinetic_f32(None, fptr(f), iptr(i0), 1, 1, 1, fptr(f), None, iptr(ws, torch.int32), stream()), "null")
    bad(L.spk_md_kinetic_f32(fptr(f), fptr(f), iptr(i0), 1, 1, 1, fptr(f), None, None, stream()), "null")
    bad(L.spk_md_nhc_global_f32(fptr(f), iptr(n1), 1, 1, 0, 2, 3, steps, 1.0, 1.0, fptr(f), fptr(f), fptr(f), stream()), "chain_length")
    bad(L.spk_md_nhc_global_f32(fptr(f), iptr(n1), 1, 1, 17, 2, 3, steps, 1.0, 1.0, fptr(f), fptr(f), fptr(f), stream()), "chain_length")
    bad(L.spk_md_nhc_global_f32(fptr(f), iptr(n1), 1, 1, 3, 2, 4, steps, 1.0, 1.0, fptr(f), fptr(f), fptr(f), stream()), "integration_order")
    bad(L.spk_md_nhc_global_f32(fptr(f), iptr(n1), 1, 1, 3, 0, 3, steps, 1.0, 1.0, fptr(f), fptr(f), fptr(f), stream()), "multi_step")
    bad(L.spk_md_nhc_global_f32(fptr(f), iptr(n1), 1, 1, 3, 2, 3, None, 1.0, 1.0, fptr(f), fptr(f), fptr(f), stream()), "sub-step")
    bad(L.spk_md_nhc_global_f32(None, iptr(n1), 1, 1, 3, 2, 3, steps, 1.0, 1.0, fptr(f), fptr(f), fptr(f), stream()), "null")
    bad(L.spk_md_nhc_massive_f32(fptr(f), None, 1, 1, 3, 2, 3, steps, 1.0, 1.0, fptr(f), fptr(f), stream()), "null")
    bad(L.spk_md_nhc_massive_f32(fptr(f), fptr(f), 1, 1, 0, 2, 3, steps, 1.0, 1.0, fptr(f), fptr(f), stream()), "chain_length")
    bad(L.spk_md_nhc_massive_f32(fptr(f), fptr(f), 1, 1, 3, 2, 2, steps, 1.0, 1.0, fptr(f), fptr(f), stream()), "integration_order")
    bad(L.spk_md_berendsen_scale_f32(fptr(f), None, 1, 1, 0.1, 1.0, 1.0, fptr(f), stream()), "null")
    bad(L.spk_md_scale_molecules_f32(fptr(f), None, iptr(i0), 1, 1, 1, None, stream()), "null")
    torch.cuda.synchronize()
    assert bool((f == 1).all())


# ----------------------------------------------------------------------------- NVTSimulation
def three_molecules():
    """Aspirin (21 atoms), ethanol (9) and a 6-atom fragment of ethanol: three molecules of different size in one batch."""
    systems = []
    for Z, R in ((S.ASPIRIN_Z, S.ASPIRIN_R), (S.ETHANOL_Z, S.ETHANOL_R), (S.ETHANOL_Z[:6], S.ETHANOL_R[:6])):
        R = np.asarray(R, dtype=np.float64)
        ii, jj = S.neighbor_pairs_open(R, 5.0)
        systems.append({"Z": list(Z), "R": R, "idx_i": ii, "idx_j": jj})
    return S.collate(systems), [21, 9, 6]


def make_thermostat(kind):
    from schnetpack_amd import md as MD
    kw = dict(fs=1.0, kb=1.0)          # the seeded models have no physical units: temperature = energy, time constant in time units
    return {"nhc": lambda: MD.NHCThermostat(0.05, 0.1, **kw), "nhc_massive": lambda: MD.NHCThermostat(0.05, 0.1, massive=True, **kw),
            "berendsen": lambda: MD.BerendsenThermostat(0.05, 0.1, **kw), "langevin": lambda: MD.LangevinThermostat(0.05, 0.1, seed=77, **kw)}[kind]()


_MODELS = {}


def nvt(dev, kind, model_kind, use_graph):
    from schnetpack_amd import model as M
    from schnetpack_amd.md import NVTSimulation
    if model_kind not in _MODELS:
        rep_p = O.init_painn_params() if model_kind == "painn" else O.init_schnet_params()
        model = M.build_model(model_kind)
        M.load_reference_params(model, rep_p, O.init_atomwise_params(128, seed=1))
        _MODELS[model_kind] = model.to(dev).eval()
    b, sizes = three_molecules()
    inp = M.batch_to_inputs(b, dev)
    inp["_n_atoms"] = torch.tensor(sizes, device=dev)
    masses = torch.where(b["Z"] == 1, 1.008, torch.where(b["Z"] == 6, 12.011, 15.999))
    sim = NVTSimulation(_MODELS[model_kind], inp, masses.to(dev), 0.02, cutoff=5.0, thermostat=make_thermostat(kind), cutoff_shell=0.3, use_graph=use_graph)
    gen = torch.Generator().manual_seed(0)
    p0 = 0.3 * torch.randn(b["R"].shape, generator=gen) * masses[:, None].sqrt()
    sim.state.momenta.copy_(p0.to(dev).unsqueeze(0))
    return sim, b, masses, p0, sizes


KINDS = ["nhc", "nhc_massive", "berendsen", "langevin"]


@pytest.mark.parametrize("kind", KINDS)
def test_nvt_graph_replay_equals_eager_bit_for_bit_and_follows_the_oracle(dev, kind):
    """Small PaiNN on three molecules of different size (molecule-resident, bit-reproducible force call): six steps as graph
    replays equal six eager steps bit for bit; and the eager run, step by step, follows the float64 oracle fed the DEVICE's own
    forces (so only the thermostat and integrator are compared) within the trajectory bars of DESIGN section 1."""
    sim_g, b, masses, p0, sizes = nvt(dev, kind, "painn", True)
    sim_e = nvt(dev, kind, "painn", False)[0]
    assert sim_g._complete and sim_g.graph is not None and sim_e.graph is None
    idx_m, n = layout(sizes)
    th = sim_e.thermostat
    m64 = masses.double()
    q, p, F = b["R"].double()[None], p0.double()[None], sim_e.state.forces.cpu().double()
    L = 3
    v = torch.zeros(1, len(m64), 3, L, dtype=torch.float64) if kind == "nhc_massive" else torch.zeros(1, 3, L, dtype=torch.float64)
    f = torch.zeros_like(v)

    def oracle_thermostat(p, step, which):
        if kind == "nhc":
            return TO.nhc_apply_global(p, m64, idx_m, n, th.kb_temperature, th.frequency, v, f, torch.tensor(th.sub_steps, dtype=torch.float64), 2)[0]
        if kind == "nhc_massive":
            return TO.nhc_apply_massive(p, m64, th.kb_temperature, th.frequency, v, f, torch.tensor(th.sub_steps, dtype=torch.float64), 2)
        if kind == "berendsen":
            ke2 = TO.kinetic_energy2(p, m64, idx_m, 3)
            T_ = ke2 / (3.0 * n[None, :].double() * th.kb)          # float64 throughout (the fixture pins the reference's float32 factor)
            return p * torch.sqrt(1.0 + 0.02 / th.time_constant * (th.temperature_bath / T_ - 1.0))[:, idx_m, None]
        c1, c2 = TO.langevin_coefficients(0.02, th.time_constant)
        return TO.langevin_apply(p, m64, c1, c2, th.kb * th.temperature_bath, MDO.pile_noise(1, len(m64), th.seed, step, which).view(1, -1, 3))
    worst_q = worst_p = 0.0
    for step in range(6):
        sim_e.step(1)
        p = TO.half_step(oracle_thermostat(p, step, 0), F, 0.02)
        q = TO.main_step(q, p, m64, 0.02)
        F = sim_e.state.forces.cpu().double()                     # the device's forces at the device's new positions
        p = oracle_thermostat(TO.half_step(p, F, 0.02), step, 1)
        worst_q, worst_p = max(worst_q, rel_err(sim_e.state.positions.cpu(), q)), max(worst_p, rel_err(sim_e.state.momenta.cpu(), p))
    print("nvt %s against the oracle on device forces: positions %.3e momenta %.3e" % (kind, worst_q, worst_p))
    assert worst_q < 1e-5 and worst_p < 1e-4
    sim_g.step(6)
    assert sim_g.step_count == 6 and sim_e.step_count == 6 and sim_g.n_captures == 1
    assert torch.equal(sim_g.state.positions, sim_e.state.positions) and torch.equal(sim_g.state.momenta, sim_e.state.momenta)
    if kind.startswith("nhc"):
        for key in ("velocities", "forces"):
            assert torch.equal(sim_g.thermostat.state_dict()[key], sim_e.thermostat.state_dict()[key])
    # per-molecule kinetic energy and temperature on the kinetic kernel
    ke = sim_g.kinetic_energy()
    ref = 0.5 * TO.kinetic_energy2(sim_g.state.momenta.cpu().double(), m64, idx_m, 3)[0]
    assert ke.shape == (3,) and rel_err(ke.cpu(), ref) < 1e-6
    assert rel_err(sim_g.temperature().cpu(), 2 * ref / (3.0 * n.double() * th.kb)) < 1e-6
    assert abs(sim_g.total_energy() - (float(sim_g.energy.sum()) + float(ref.sum()))) < 1e-4 * float(ref.sum())


@pytest.mark.parametrize("kind", KINDS)
def test_nvt_schnet_graph_replay_follows_eager(dev, kind):
    """The same with SchNet (its force call sums with atomics): graph against eager within the trajectory bars of DESIGN section 1."""
    sim_g = nvt(dev, kind, "schnet", True)[0]
    sim_e = nvt(dev, kind, "schnet", False)[0]
    sim_g.step(6)
    sim_e.step(6)
    eq, ep = rel_err(sim_g.state.positions, sim_e.state.positions), rel_err(sim_g.state.momenta, sim_e.state.momenta)
    print("nvt schnet %s graph against eager: positions %.3e momenta %.3e" % (kind, eq, ep))
    assert eq < 1e-5 and ep < 1e-4


def test_nvt_periodic_run_keeps_chain_state_and_step_counter_across_rebuilds(dev):
    """Periodic 192-atom water box, PaiNN, NHC: hot start, the skin criterion forces list rebuilds (= graph re-captures) mid-run.
    The re-captured step keeps using the SAME chain-state and step-counter tensors: the counter equals the number of steps, the
    chain has moved and is finite, the thermostat cools the hot box."""
    from schnetpack_amd import md as MD, model as M
    model = M.build_model("painn")
    M.load_reference_params(model, O.init_painn_params(), O.init_atomwise_params(128, seed=1))
    model = model.to(dev).eval()
    b = S.water_box(n_side=4, seed=7)
    inp = M.batch_to_inputs(b, dev)
    inp["_n_atoms"] = torch.tensor([b["Z"].shape[0]], device=dev)
    inp["_cell"] = b["cell"].reshape(1, 3, 3).to(dev)
    inp["_pbc"] = torch.tensor([True, True, True], device=dev)
    masses = torch.where(b["Z"] == 1, 1.008, 15.999)
    th = MD.NHCThermostat(0.05, 0.3, fs=1.0, kb=1.0)
    sim = MD.NVTSimulation(model, inp, masses.to(dev), 0.01, cutoff=5.0, thermostat=th, cutoff_shell=0.3)
    gen = torch.Generator().manual_seed(1)
    sim.state.momenta.copy_((0.7 * torch.randn(b["R"].shape, generator=gen) * masses[:, None].sqrt()).to(dev).unsqueeze(0))
    t0 = float(sim.temperature()[0])
    ptr_v, ptr_c = th._vel.data_ptr(), sim._stepc.data_ptr()
    sim.step(200)
    assert sim.nl.n_builds >= 2 and sim.n_captures >= 2, (sim.nl.n_builds, sim.n_captures)
    assert sim.step_count == 200 and th._vel.data_ptr() == ptr_v and sim._stepc.data_ptr() == ptr_c
    sd = th.state_dict()
    assert bool(torch.isfinite(sd["velocities"]).all()) and float(sd["velocities"].abs().max()) > 0
    t1 = float(sim.temperature()[0])
    print("nvt water box: %d list builds, %d captures, temperature %.4f -> %.4f (bath 0.05)" % (sim.nl.n_builds, sim.n_captures, t0, t1))
    assert t1 < t0
