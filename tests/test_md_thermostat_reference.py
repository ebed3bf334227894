"""CPU: the classical thermostats (Berendsen, Langevin, Nose-Hoover chain; md/simulation_hooks/thermostats.py of the reference)
against tests/golden/md_thermostat.npz, which tests/make_md_thermostat_golden.py produces by executing the reference's OWN lifted
methods.  Pinned here: tests/md_thermostat_oracle.py (the float64 restatement the GPU tests compare with: 1e-12 against the
fixture) and the host side of ``schnetpack_amd.md`` -- coefficients, thermostat masses, Yoshida-Suzuki sub-steps, the step order of
``NVTSimulation``, the ``state_dict`` round trip -- driven by a host stand-in for the device entries.

The fixture's float64 runs carry the reference's float32-rounded buffers (time constant, frequency, kT: python floats registered
as float32 tensors); they are stored and handed to the oracle, so 1e-12 holds.  The host classes use float64 constants and are
held to the tolerance rule of the device (``md_thermostat_oracle.allowed_error``).  Unit constants are not pinned.
"""
import types

import numpy as np
import pytest
import torch

from conftest import load_npz, rel_err
from oracle import md_oracle as MDO
from oracle import refshim

import md_thermostat_oracle as TO

APPS = (1, 2, 6)
KINDS = ("nhc_global", "nhc_massive", "berendsen", "langevin")
# NVTSimulation on the host in float64 against the reference's float64 trajectory: the reference's constants are float32-rounded
# (2^-24 relative) and enter each of the 12 thermostat applications of six steps once
SIM_TOL = 12 * 2.0 ** -24


@pytest.fixture(scope="module")
def g():
    return load_npz("md_thermostat.npz")


def T(x):
    return torch.from_numpy(np.asarray(x))


def nhc_cases(g=None):
    import make_md_thermostat_golden as G
    return [c[0] for c in G.NHC_CASES]


def system(g):
    return T(g["p"]), T(g["masses"]).reshape(-1), T(g["idx_m"]), T(g["n_atoms"])


def rel(a, b):
    return rel_err(a.reshape(b.shape), b)


# ----------------------------------------------------------------------------- fixture and oracle
def test_fixture_holds_the_stated_cases(g):
    from schnetpack_amd import md as MD
    assert list(g["n_atoms"]) == [2, 5, 9] and int(g["n_replicas"]) == 2 and tuple(g["applications"]) == APPS
    assert (g["unit_kB"], g["unit_fs"]) == (MD.KB_MD, MD.FS_MD)
    params = {str(t): tuple(int(x) for x in r) for t, r in zip(g["nhc_cases"], g["nhc_params"])}
    assert {p[0] for p in params.values()} >= {1, 2, 3, 6} and {p[1] for p in params.values()} >= {1, 2, 4} and {p[2] for p in params.values()} == {1, 3, 5, 7}
    assert {p[3] for p in params.values()} == {0, 1}
    assert g["p"].dtype == np.float64 and g["p"].shape == (2, 16, 3)
    m = g["masses"].reshape(-1)
    assert m[0] == 1.008 and m[1] == 200.0
    assert float(g["temperature"].max()) > 2 * float(g["temperature_bath"])            # the thermostats have work to do


def test_oracle_kinetic_energy_and_temperature(g):
    p, m, idx_m, n = system(g)
    ke2 = TO.kinetic_energy2(p, m, idx_m, 3)
    assert rel(ke2, T(g["ke2"])) < 1e-12
    assert rel(TO.temperature(ke2, n, float(g["unit_kB"])), T(g["temperature"])) < 1e-12


@pytest.mark.parametrize("tag", nhc_cases())
def test_oracle_nhc_matches_the_reference(g, tag):
    """Scale, chain velocities and forces, momenta after 1, 2 and 6 consecutive applications: 1e-12 relative."""
    p, m, idx_m, n = system(g)
    L, ms, order, massive = (int(x) for x in g["nhc_params"][list(g["nhc_cases"]).index(tag)])
    kT, freq, steps, tm = float(g["nhc_%s_kT" % tag]), float(g["nhc_%s_frequency" % tag]), T(g["nhc_%s_steps" % tag]), T(g["nhc_%s_masses" % tag])
    assert steps.shape == (order,)
    v = torch.zeros(2, 16, 3, L, dtype=torch.float64) if massive else torch.zeros(2, 3, L, dtype=torch.float64)
    f = torch.zeros_like(v)
    for k in range(1, 7):
        if massive:
            p_new = TO.nhc_apply_massive(p, m, kT, freq, v, f, steps, ms, tm)
            s = p_new / p
        else:
            p_new, s = TO.nhc_apply_global(p, m, idx_m, n, kT, freq, v, f, steps, ms, tm.squeeze(2))
        p = p_new
        if k in APPS:
            t = "nhc_%s_f64_" % tag
            for name, got in (("scale", s), ("v", v), ("f", f), ("p", p)):
                assert rel(got, T(g[t + "%s_%d" % (name, k)])) < 1e-12, (name, k)


def test_oracle_berendsen_and_langevin_match_the_reference(g):
    p, m, idx_m, n = system(g)
    q = p
    for k in range(1, 7):
        q, _ = TO.berendsen_apply(q, m, idx_m, n, float(g["dt"]), float(g["ber_tau"]), float(g["temperature_bath"]), float(g["unit_kB"]))
        if k in APPS:
            assert rel(q, T(g["ber_p_%d" % k])) < 1e-12
    xi = MDO.pile_noise(1, 32, int(g["seed"]), 0, 0).view(2, 16, 3)
    assert torch.equal(xi, T(g["lan_noise"]))
    c1, c2 = TO.langevin_coefficients(float(g["dt"]), float(g["lan_tau"]))
    assert abs(c1 - float(g["lan_f64_c1"][0])) < 1e-14 and abs(c2 - float(g["lan_f64_c2"][0])) < 1e-13
    out = TO.langevin_apply(p, m, c1, c2, float(g["unit_kB"]) * float(g["temperature_bath"]), xi)
    assert rel(out, T(g["lan_f64_p_out"])) < 1e-12
    assert rel(T(g["lan_f32_p_out"]), T(g["lan_f64_p_out"])) < 64 * 2.0 ** -24


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_trajectory_follows_the_reference_simulator(g, kind):
    """Six steps of the lifted ``Simulator.simulate`` + ``VelocityVerlet`` + hook: event order, and the stored wrong order
    (thermostat after the first half step) is at least 100x the tolerance of the host-class test away."""
    assert list(g["sim_%s_events" % kind]) == ["calculate", "thermostat", "half_step", "main_step", "calculate", "half_step", "thermostat"]
    q, p = T(g["sim_%s_q" % kind]), T(g["sim_%s_p" % kind])
    assert q.shape == (6, 2, 16, 3)
    assert rel(T(g["sim_%s_wrong_q" % kind]), q[-1]) >= 100 * SIM_TOL and rel(T(g["sim_%s_wrong_p" % kind]), p[-1]) >= 100 * SIM_TOL


@pytest.mark.skipif(not (refshim.available() and not refshim.sourceless()), reason="reference sources not present (the fixture is regenerated from them)")
def test_fixture_is_what_the_reference_produces_now(g, tmp_path):
    """Regenerated in memory from the live reference (which also re-checks the oracle trajectories at 1e-12): same keys, dtypes,
    values, and the same bytes when written."""
    import os
    from conftest import GOLDEN
    import make_md_thermostat_golden as G
    fresh = G.arrays()
    stored = np.load(os.path.join(GOLDEN, "md_thermostat.npz"), allow_pickle=False)
    assert sorted(fresh) == sorted(stored.files)
    for k, v in fresh.items():
        v = np.asanyarray(v)
        assert v.dtype == stored[k].dtype and v.shape == stored[k].shape and np.array_equal(v, stored[k]), k
        assert v.dtype.kind in "fiubU", k
    G.save_npz_reproducible(str(tmp_path / "again.npz"), fresh)
    assert (tmp_path / "again.npz").read_bytes() == open(os.path.join(GOLDEN, "md_thermostat.npz"), "rb").read()


# ----------------------------------------------------------------------------- host classes on a host stand-in
def host_state(g, dtype=torch.float64):
    from schnetpack_amd import md as MD
    p, m, idx_m, n = system(g)
    return MD.MDState(T(g["q"]).to(dtype).clone(), p.to(dtype).clone(), m.to(dtype).reshape(1, -1, 1)), idx_m, n


def make_nhc(g, tag, **kw):
    from schnetpack_amd import md as MD
    L, ms, order, massive = (int(x) for x in g["nhc_params"][list(g["nhc_cases"]).index(tag)])
    return MD.NHCThermostat(float(g["temperature_bath"]), float(g["tau_fs"]), L, bool(massive), ms, order, compute_fn=TO.HostCompute, **kw)


@pytest.mark.parametrize("tag", nhc_cases())
def test_nhc_class_constants_and_application(g, tag):
    """Sub-steps and thermostat masses within 4 float32 ulp of the reference's (float32-derived) values; scale, chain state and
    momenta after 1, 2, 6 applications within the device's tolerance rule of the reference's float64 run; state_dict in the
    reference's buffer names and shapes."""
    state, idx_m, n = host_state(g)
    th = make_nhc(g, tag).init(types.SimpleNamespace(time_step=float(g["dt"])), idx_m, n)
    steps = T(g["nhc_%s_steps" % tag])
    assert bool(((torch.tensor(th.sub_steps, dtype=torch.float64) - steps).abs() <= 4 * TO.U23 * steps.abs()).all())
    assert abs(th.kb_temperature - float(g["nhc_%s_kT" % tag])) <= 4 * TO.U23 * th.kb_temperature
    p0 = state.momenta.clone()
    for k in range(1, 7):
        before = state.momenta.clone()
        th.apply(state, 0, 0)
        if k == 1:
            tm = T(g["nhc_%s_masses" % tag])
            assert th.masses.shape == tm.shape and bool(((th.masses - tm).abs() <= 4 * TO.U23 * tm.abs()).all())
            assert bool((th.degrees_of_freedom == T(g["nhc_%s_dof" % tag])).all())
        if k in APPS:
            sd = th.state_dict()
            assert sorted(sd) == ["forces", "masses", "velocities"]
            scale = (state.momenta / before) if th.massive else th.scaling_factor
            for name, got in (("scale", scale), ("v", sd["velocities"]), ("f", sd["forces"]), ("p", state.momenta)):
                r64, r32 = T(g["nhc_%s_f64_%s_%d" % (tag, name, k)]), T(g["nhc_%s_f32_%s_%d" % (tag, name, k)])
                assert got.numel() == r64.numel() and (name in ("scale", "p") or got.shape == r64.shape)
                err = float((got.reshape(r64.shape) - r64).abs().max())
                assert err <= TO.allowed_error(r64, r32), (name, k, err, TO.allowed_error(r64, r32))
    assert not torch.equal(p0, state.momenta)


@pytest.mark.parametrize("tag", ["g_l3_m2_o3", "m_l3_m2_o3", "g_l1_m1_o3"])
def test_nhc_state_dict_continues_a_trajectory_bit_identically(g, tag):
    state, idx_m, n = host_state(g, torch.float32)
    integ = types.SimpleNamespace(time_step=float(g["dt"]))
    th = make_nhc(g, tag).init(integ, idx_m, n)
    for _ in range(3):
        th.apply(state)
    sd = {k: v.clone() for k, v in th.state_dict().items()}
    p_mid = state.momenta.clone()
    for _ in range(3):
        th.apply(state)
    from schnetpack_amd import md as MD
    state2 = MD.MDState(state.positions, p_mid.clone(), state.masses)
    for early in (True, False):                         # loaded before the buffers exist, and into existing buffers
        th2 = make_nhc(g, tag).init(integ, idx_m, n)
        st = MD.MDState(state.positions, p_mid.clone(), state.masses)
        if not early:
            th2._prepare(st)
        th2.load_state_dict(sd)
        for _ in range(3):
            th2.apply(st)
        assert torch.equal(st.momenta, state.momenta)
        for k in ("velocities", "forces"):
            assert torch.equal(th2.state_dict()[k], th.state_dict()[k])
    assert not torch.equal(state2.momenta, state.momenta)
    bad = dict(sd, masses=2 * sd["masses"])
    with pytest.raises(ValueError, match="masses"):
        th2.load_state_dict(bad)


def test_berendsen_class_matches_the_reference(g):
    from schnetpack_amd import md as MD
    state, idx_m, n = host_state(g)
    th = MD.BerendsenThermostat(float(g["temperature_bath"]), float(g["tau_fs"]), compute_fn=TO.HostCompute).init(types.SimpleNamespace(time_step=float(g["dt"])), idx_m, n)
    assert abs(th.time_constant - float(g["ber_tau"])) <= TO.U23 * th.time_constant
    for k in range(1, 7):
        th.apply(state)
        if k in APPS:
            r64, r32 = T(g["ber_p_%d" % k]), T(g["ber_f32_p_%d" % k])
            assert float((state.momenta - r64).abs().max()) <= TO.allowed_error(r64, r32)
    # a molecule at rest and a molecule without atoms keep their momenta (the reference yields NaN)
    p = torch.zeros(1, 4, 3, dtype=torch.float64)
    p[0, 2:] = 1.0
    st = MD.MDState(p.clone(), p.clone(), torch.ones(1, 4, 1, dtype=torch.float64))
    th.init(types.SimpleNamespace(time_step=1e-3), torch.tensor([0, 0, 2, 2]), torch.tensor([2, 0, 2])).apply(st)
    assert bool(torch.isfinite(st.momenta).all()) and torch.equal(st.momenta[0, :2], p[0, :2]) and not torch.equal(st.momenta[0, 2:], p[0, 2:])


def test_langevin_class_is_the_one_bead_pile_thermostat(g):
    """c1, c2 of the reference; M and noise_scale EXACTLY those of PILE-L at one bead (whose centroid friction 1 / time_constant does
    not depend on omega); the application on the noise of (seed, step, which) against the reference's float64 run."""
    from schnetpack_amd import md as MD
    dt, tau_fs, T0 = float(g["dt"]), float(g["tau_fs"]), float(g["temperature_bath"])
    state, idx_m, n = host_state(g)
    th = MD.LangevinThermostat(T0, tau_fs, seed=int(g["seed"]), compute_fn=TO.host_pile(MDO.pile_noise)).init(types.SimpleNamespace(time_step=dt))
    for name in ("c1", "c2"):
        r32, r64 = float(g["lan_f32_" + name][0]), float(g["lan_f64_" + name][0])
        assert abs(float(getattr(th, name)) - r64) <= max(4 * abs(r32 - r64), 4 * TO.U23 * r64)
    for omega in (0.5, 40.0, 3000.0):
        pile = MD.PILELocalThermostat(T0, tau_fs).init(MD.RingPolymer(dt, 1, T0, omega=omega))
        assert torch.equal(pile.M, th.M) and pile.noise_scale == th.noise_scale
        assert torch.equal(MD.pile_matrices(1, omega, dt, tau_fs * MD.FS_MD), th.M)
    th.apply(state, 0, 0)
    r64, r32 = T(g["lan_f64_p_out"]), T(g["lan_f32_p_out"])
    assert float((state.momenta - r64).abs().max()) <= TO.allowed_error(r64, r32)
    # the step comes from the device word when one is given
    st2, _, _ = host_state(g)
    th.apply(st2, 5, 0, torch.zeros(1, dtype=torch.int64))
    assert torch.equal(st2.momenta, state.momenta)


class HostVerlet:
    """``VelocityVerlet`` of schnetpack_amd.md on host tensors, in place, logging what it is asked to do."""
    ring_polymer = False

    def __init__(self, time_step, events):
        self.time_step, self.events = time_step, events

    def half_step(self, state):
        self.events.append("half_step")
        state.momenta.add_(0.5 * self.time_step * state.forces)

    def first_half_and_main_step(self, state, kick=True, *skin):
        assert kick
        self.events.append("half_step+main_step")
        state.momenta.add_(0.5 * self.time_step * state.forces)
        state.positions.add_(self.time_step * state.momenta / state.masses)


@pytest.mark.parametrize("kind", KINDS)
def test_nvt_simulation_step_order_on_a_stub_force_function(g, kind):
    """``NVTSimulation._step_body`` (the parent's kick-drift / force call / kick between two thermostat applications, then the step
    counter) on host tensors, a host integrator and the fixture's harmonic forces: the trajectory of the reference's
    ``Simulator.simulate``.  The stored wrong order is >= 100 SIM_TOL away (test above), so this sees a swapped pair."""
    from schnetpack_amd import md as MD
    import make_md_thermostat_golden as G
    dt, tau_fs, T0 = float(g["dt"]), float(g["tau_fs"]), float(g["temperature_bath"])
    state, idx_m, n = host_state(g)
    events = []
    th = {"nhc_global": lambda: MD.NHCThermostat(T0, tau_fs, compute_fn=TO.HostCompute),
          "nhc_massive": lambda: MD.NHCThermostat(T0, tau_fs, massive=True, compute_fn=TO.HostCompute),
          "berendsen": lambda: MD.BerendsenThermostat(T0, tau_fs, compute_fn=TO.HostCompute),
          "langevin": lambda: MD.LangevinThermostat(T0, tau_fs, seed=int(g["seed"]), compute_fn=TO.host_pile(MDO.pile_noise))}[kind]()
    apply = th.apply
    th.apply = lambda *a, **k: (events.append("thermostat"), apply(*a, **k))[1]
    sim = MD.NVTSimulation.__new__(MD.NVTSimulation)
    sim.state, sim.integrator, sim.thermostat, sim._complete = state, HostVerlet(dt, events), th, True
    sim._stepc = torch.zeros(1, dtype=torch.int64)
    th.init(sim, idx_m, n)

    def force_eval():
        events.append("calculate")
        state.forces = G.spring_forces(state.positions, idx_m)
    sim._force_eval = force_eval
    force_eval()
    q_ref, p_ref = T(g["sim_%s_q" % kind]), T(g["sim_%s_p" % kind])
    for k in range(6):
        sim._step_body()
        assert rel(state.positions, q_ref[k]) <= SIM_TOL and rel(state.momenta, p_ref[k]) <= SIM_TOL, k
    assert events[:6] == ["calculate", "thermostat", "half_step+main_step", "calculate", "half_step", "thermostat"]
    assert sim.step_count == 6


def test_out_of_scope_combinations_are_refused():
    from schnetpack_amd import md as MD
    rp = MD.RingPolymer(1e-3, 4, 300.0)
    for th in (MD.BerendsenThermostat(300.0, 100.0), MD.LangevinThermostat(300.0, 100.0), MD.NHCThermostat(300.0, 100.0)):
        assert th.ring_polymer is False
        with pytest.raises(ValueError, match="ring"):
            th.init(rp)
    with pytest.raises(ValueError, match="ring-polymer"):
        MD.NVTSimulation(None, {}, None, 1e-3, 5.0, thermostat=MD.PILELocalThermostat(300.0, 100.0))
    with pytest.raises(NotImplementedError, match="barostat"):
        MD.NVTSimulation(None, {}, None, 1e-3, 5.0, barostat=object())
    with pytest.raises(NotImplementedError, match="GLE"):
        MD.NVTSimulation(None, {}, None, 1e-3, 5.0, thermostat=object())
    with pytest.raises(ValueError):
        MD.NHCThermostat(300.0, 100.0, chain_length=0)
    with pytest.raises(ValueError):
        MD.NHCThermostat(300.0, 100.0, integration_order=4)
    with pytest.raises(ValueError):
        MD.NHCThermostat(300.0, 100.0, multi_step=0)
    with pytest.raises(ValueError, match="ascend"):
        MD.NHCThermostat(300.0, 100.0).init(types.SimpleNamespace(time_step=1e-3), torch.tensor([1, 0]), torch.tensor([1, 1]))
    import inspect
    sig = inspect.signature(MD.NHCThermostat.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[3:7]] == [("chain_length", 3), ("massive", False), ("multi_step", 2), ("integration_order", 3)]
    for name in ("BerendsenThermostat", "LangevinThermostat", "NHCThermostat", "NVTSimulation"):
        assert name in MD.__all__


def test_header_declares_the_thermostat_entries():
    """The existing header test (tests/test_host_logic.py) resolves every declared symbol in the built library and in the ctypes
    table; this pins that the new entries are among the declared ones."""
    from test_host_logic import header_functions
    from schnetpack_amd import _lib
    names = {"spk_md_kinetic_workspace_bytes", "spk_md_kinetic_f32", "spk_md_nhc_global_f32", "spk_md_nhc_massive_f32",
             "spk_md_berendsen_scale_f32", "spk_md_scale_molecules_f32"}
    assert names <= set(header_functions()) and names <= set(_lib.exported_symbols())
