"""Generator of tests/golden/md_thermostat.npz (a plain script, not collected by pytest):

    python tests/make_md_thermostat_golden.py

It lifts, with ``ast`` at run time, the reference's own ``NHCThermostat`` (``_init_thermostat``, ``_init_masses``,
``_propagate_thermostat``, ``_compute_kinetic_energy``, ``_apply_thermostat``), ``BerendsenThermostat._apply_thermostat``,
``LangevinThermostat`` (``_init_thermostat``, ``_apply_thermostat``), ``YSWeights``, ``System.kinetic_energy`` / ``temperature`` /
``sum_atoms`` / ``expand_atoms``, ``VelocityVerlet`` and ``Simulator.simulate`` and stores ONLY the arrays they compute.  Every
NHC case is evaluated twice, on a float64 and on a float32 system: the difference is the reference's own float32 gap, the
yardstick of the device tolerances.  Unit constants: the project's (stored as ``unit_*``), not pinned.

The hooks' buffers are those of ``ThermostatHook.__init__`` / ``NHCThermostat.__init__`` / ``LangevinThermostat.__init__`` (python
floats become float32 tensors, as ``register_buffer(torch.tensor(x))`` makes them) and ``to(dtype)`` casts the floating ones like
``nn.Module.to``: the float64 run therefore carries the reference's float32-rounded time constant, frequency and kT, which are
stored (``*_kT``, ``*_frequency``, ``*_steps``) so that a float64 restatement can be pinned to 1e-12.

Integration order 1 is not in the reference's weight table; those cases run the lifted code with the weight table extended by
the trivial entry {1: [1.0]} (one unsplit sub-step).
"""
import ast
import os
import sys
import types
from contextlib import nullcontext

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import md_oracle as MDO  # noqa: E402
from oracle.make_golden import _TorchWithNoise, _lift, _md_path, _md_units, save_npz_reproducible  # noqa: E402
import md_thermostat_oracle as TO  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "md_thermostat.npz")

N_ATOMS_MOL = [2, 5, 9]          # three molecules of different size
N_REPLICAS = 2
T_BATH, T_START = 300.0, 600.0   # momenta drawn at twice the bath temperature: the thermostats have work to do
DT = 2.0e-3                      # 2 fs in ps
TAU_FS = 10.0                    # omega dt = 0.2: a few per cent of scaling per application
APPLICATIONS = (1, 2, 6)
# (tag, chain_length, multi_step, integration_order, massive)
NHC_CASES = [("g_l3_m2_o3", 3, 2, 3, False), ("g_l1_m1_o3", 1, 1, 3, False), ("g_l2_m4_o5", 2, 4, 5, False), ("g_l6_m2_o7", 6, 2, 7, False),
             ("g_l3_m1_o1", 3, 1, 1, False), ("g_l6_m4_o1", 6, 4, 1, False),
             ("m_l3_m2_o3", 3, 2, 3, True), ("m_l1_m2_o3", 1, 2, 3, True), ("m_l6_m1_o5", 6, 1, 5, True), ("m_l2_m4_o7", 2, 4, 7, True)]
SEED = 0xBADC0FFEE
SIM_STEPS = 6
SPRING_K, SPRING_R0 = 300.0, 0.15          # harmonic pair potential inside every molecule (kJ/mol/nm^2, nm)


def _lift_class(path, cls, env):
    """The class ``cls`` of the reference file ``path`` compiled in memory against ``env`` (annotations dropped)."""
    tree = ast.parse(open(path).read())
    node = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls][0]
    for fn in node.body:
        if isinstance(fn, ast.FunctionDef):
            fn.returns = None
            for a in fn.args.args + fn.args.kwonlyargs:
                a.annotation = None
    exec(compile(ast.Module([node], []), os.path.basename(path), "exec"), env)
    return env[cls]


def ys_weights_class():
    ys = _lift_class(_md_path("utils", "thermostat_utils.py"), "YSWeights", {"torch": torch})
    assert sorted(ys.YS_weights) == [3, 5, 7]
    table = dict(ys.YS_weights)
    table[1] = torch.tensor([1.0], dtype=torch.float64)
    return type("YSWeightsWithOrder1", (ys,), {"YS_weights": table})


def system_class():
    env = {"torch": torch, "spk_units": _md_units()}
    fns = _lift(_md_path("system.py"), "System", ("kinetic_energy", "temperature", "sum_atoms", "expand_atoms"), env)

    def __init__(self, q, p, m, n_atoms_mol, forces=None):
        self.positions, self.momenta, self.masses, self.forces = q, p, m, forces
        self.n_replicas, self.n_atoms = int(p.shape[0]), n_atoms_mol
        self.n_molecules, self.total_n_atoms = int(n_atoms_mol.shape[0]), int(n_atoms_mol.sum())
        self.index_m = torch.repeat_interleave(torch.arange(self.n_molecules), n_atoms_mol)
    return type("LiftedSystem", (), {"__init__": __init__, "sum_atoms": fns["sum_atoms"], "expand_atoms": fns["expand_atoms"],
                                     "kinetic_energy": property(fns["kinetic_energy"]), "temperature": property(fns["temperature"])})


def _to(self, arg):
    """nn.Module.to on the registered buffers: floating tensors follow a dtype, a device changes nothing here."""
    if isinstance(arg, torch.dtype):
        for k, v in list(self.__dict__.items()):
            if isinstance(v, torch.Tensor) and v.is_floating_point():
                self.__dict__[k] = v.to(arg)
    return self


def hook_class(kind, noise=()):
    units = _md_units()
    env = {"torch": _TorchWithNoise(noise) if kind == "langevin" else torch, "spk_units": units, "YSWeights": ys_weights_class()}
    fns = _lift(_md_path("simulation_hooks", "basic_hooks.py"), "SimulationHook",
                ("on_step_begin", "on_step_middle", "on_step_end", "on_step_finalize", "on_simulation_start", "on_simulation_end"), env)
    fns.update(_lift(_md_path("simulation_hooks", "thermostats.py"), "ThermostatHook", ("on_simulation_start", "on_step_begin", "on_step_end"), env))
    path = _md_path("simulation_hooks", "thermostats.py")
    if kind == "nhc":
        fns.update(_lift(path, "NHCThermostat", ("_init_thermostat", "_init_masses", "_propagate_thermostat", "_compute_kinetic_energy", "_apply_thermostat"), env))
    elif kind == "berendsen":
        fns.update(_lift(path, "BerendsenThermostat", ("_apply_thermostat",), env))
        fns["_init_thermostat"] = lambda self, simulator: None            # ThermostatHook._init_thermostat: pass
    else:
        fns.update(_lift(path, "LangevinThermostat", ("_init_thermostat", "_apply_thermostat"), env))

    def __init__(self, temperature_bath, time_constant, chain_length=3, massive=False, multi_step=2, integration_order=3):
        self.temperature_bath = torch.tensor(temperature_bath)
        self.time_constant = torch.tensor(time_constant * units.fs)
        self.initialized = False
        if kind == "nhc":
            self.chain_length, self.massive = torch.tensor(chain_length), torch.tensor(massive)
            self.frequency = 1.0 / self.time_constant
            self.kb_temperature = self.temperature_bath * units.kB
            self.multi_step, self.integration_order = torch.tensor(multi_step), torch.tensor(integration_order)
    fns["__init__"] = __init__
    fns["to"] = _to
    return type("Lifted_" + kind, (), fns)


def base_system():
    """Masses in [1, 16] with a hydrogen and a heavy atom, thermal momenta at T_START, positions on a jittered lattice (float64)."""
    n_mol = torch.tensor(N_ATOMS_MOL)
    N = int(n_mol.sum())
    g = torch.Generator().manual_seed(77)
    m = torch.rand(1, N, 1, generator=g, dtype=torch.float64) * 15 + 1
    m[0, 0, 0], m[0, 1, 0] = 1.008, 200.0
    p = torch.randn(N_REPLICAS, N, 3, generator=g, dtype=torch.float64) * (m * _md_units().kB * T_START).sqrt()
    q = 0.12 * torch.stack(torch.meshgrid(torch.arange(4.), torch.arange(2.), torch.arange(2.), indexing="ij"), -1).reshape(-1, 3).double()
    q = q[None].repeat(N_REPLICAS, 1, 1) + 0.01 * torch.randn(N_REPLICAS, N, 3, generator=g, dtype=torch.float64)
    return n_mol, m, p, q


def spring_forces(q, idx_m):
    """-dE/dq of E = k/2 sum over the pairs i < j of one molecule of (|q_i - q_j| - r0)^2, analytic."""
    d = q[:, :, None, :] - q[:, None, :, :]
    r = d.norm(dim=-1)
    same = (idx_m[:, None] == idx_m[None, :]) & ~torch.eye(len(idx_m), dtype=torch.bool)
    w = torch.where(same, -SPRING_K * (r - SPRING_R0) / r.clamp_min(1e-30), torch.zeros_like(r))
    return (w[..., None] * d).sum(2)


def simulator_for(system, dtype):
    return types.SimpleNamespace(system=system, integrator=types.SimpleNamespace(time_step=DT), device=torch.device("cpu"), dtype=dtype)


def record_nhc(arrs):
    """NHC cases: scale, chain velocities / forces and momenta after 1, 2 and 6 consecutive applications, float64 and float32."""
    System = system_class()
    n_mol, m, p, q = base_system()
    for tag, L, ms, order, massive in NHC_CASES:
        for dt_tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            th = hook_class("nhc")(T_BATH, TAU_FS, L, massive, ms, order)
            system = System(None, p.to(dtype).clone(), m.to(dtype), n_mol)
            sim = simulator_for(system, dtype)
            th.on_simulation_start(sim)
            assert th.velocities.dtype == dtype and th.masses.dtype == dtype and th.time_step.dtype == dtype
            scales = []
            propagate = type(th)._propagate_thermostat
            th._propagate_thermostat = lambda ke, th=th: scales.append(propagate(th, ke)) or scales[-1]
            t = "nhc_%s_%s_" % (tag, dt_tag)
            if dt_tag == "f64":
                arrs.update({"nhc_%s_kT" % tag: th.kb_temperature.numpy().copy(), "nhc_%s_frequency" % tag: th.frequency.numpy().copy(),
                             "nhc_%s_steps" % tag: th.time_step.numpy().copy(), "nhc_%s_masses" % tag: th.masses.numpy().copy(),
                             "nhc_%s_dof" % tag: th.degrees_of_freedom.numpy().copy()})
            for k in range(1, max(APPLICATIONS) + 1):
                th.on_step_begin(sim)
                if k in APPLICATIONS:
                    s = scales[-1]
                    assert s.dtype == dtype and system.momenta.dtype == dtype
                    arrs.update({t + "scale_%d" % k: s.double().numpy().copy(), t + "v_%d" % k: th.velocities.double().numpy().copy(),
                                 t + "f_%d" % k: th.forces.double().numpy().copy(), t + "p_%d" % k: system.momenta.double().numpy().copy()})
            assert len(scales) == max(APPLICATIONS)


def record_system(arrs):
    System = system_class()
    n_mol, m, p, q = base_system()
    system = System(q, p, m, n_mol)
    arrs.update({"n_atoms": n_mol.numpy(), "masses": m.numpy(), "p": p.numpy(), "q": q.numpy(), "idx_m": system.index_m.numpy(),
                 "ke2": (2.0 * system.kinetic_energy).numpy(), "temperature": system.temperature.numpy()})


def record_berendsen(arrs):
    System = system_class()
    n_mol, m, p, q = base_system()
    for t, dtype in (("ber_", torch.float64), ("ber_f32_", torch.float32)):
        th = hook_class("berendsen")(T_BATH, TAU_FS)
        system = System(None, p.to(dtype).clone(), m.to(dtype), n_mol)
        sim = simulator_for(system, dtype)
        th.on_simulation_start(sim)
        arrs["ber_tau"] = th.time_constant.double().numpy().copy()
        for k in range(1, max(APPLICATIONS) + 1):
            th.on_step_begin(sim)
            assert system.momenta.dtype == dtype
            if k in APPLICATIONS:
                arrs[t + "p_%d" % k] = system.momenta.double().numpy().copy()


def langevin_noise(step, which, n_rep, N):
    return MDO.pile_noise(1, n_rep * N, SEED, step, which).view(n_rep, N, 3)


def record_langevin(arrs):
    System = system_class()
    n_mol, m, p, q = base_system()
    N = int(n_mol.sum())
    xi = langevin_noise(0, 0, N_REPLICAS, N)
    for dt_tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        th = hook_class("langevin", [xi])(T_BATH, TAU_FS)
        system = System(None, p.to(dtype).clone(), m.to(dtype), n_mol)
        sim = simulator_for(system, dtype)
        th.on_simulation_start(sim)
        th.on_step_begin(sim)
        assert system.momenta.dtype == dtype
        arrs.update({"lan_%s_c1" % dt_tag: th.c1.double().reshape(-1).numpy().copy(), "lan_%s_c2" % dt_tag: th.c2.double().reshape(-1).numpy().copy(),
                     "lan_%s_p_out" % dt_tag: system.momenta.double().numpy().copy()})
    arrs.update({"lan_noise": xi.numpy(), "lan_tau": th.time_constant.double().numpy().copy()})


def oracle_trajectory(kind, order, consts):
    """Six steps through tests/md_thermostat_oracle.py; ``order``: "reference" or "after_half_step" (the thermostat of the step
    begin applied AFTER the first half step: the wrong order the fixture must tell apart)."""
    n_mol, m, p, q = base_system()
    m1, idx_m = m.reshape(-1), torch.repeat_interleave(torch.arange(len(N_ATOMS_MOL)), n_mol)
    N = int(n_mol.sum())
    L = 3
    v = torch.zeros(N_REPLICAS, N, 3, L, dtype=torch.float64) if kind == "nhc_massive" else torch.zeros(N_REPLICAS, len(N_ATOMS_MOL), L, dtype=torch.float64)
    f = torch.zeros_like(v)

    def thermostat(p, step, which):
        if kind == "nhc_global":
            return TO.nhc_apply_global(p, m1, idx_m, n_mol, consts["kT"], consts["frequency"], v, f, consts["steps"], 2, consts["m"])[0]
        if kind == "nhc_massive":
            return TO.nhc_apply_massive(p, m1, consts["kT"], consts["frequency"], v, f, consts["steps"], 2, consts["m"])
        if kind == "berendsen":
            return TO.berendsen_apply(p, m1, idx_m, n_mol, DT, consts["tau"], T_BATH, _md_units().kB)[0]
        return TO.langevin_apply(p, m1, consts["c1"], consts["c2"], _md_units().kB * T_BATH, langevin_noise(step, which, N_REPLICAS, N))
    F = spring_forces(q, idx_m)
    qs, ps = [], []
    for step in range(SIM_STEPS):
        if order == "reference":
            p = TO.half_step(thermostat(p, step, 0), F, DT)
        else:
            p = thermostat(TO.half_step(p, F, DT), step, 0)
        q = TO.main_step(q, p, m1, DT)
        F = spring_forces(q, idx_m)
        p = thermostat(TO.half_step(p, F, DT), step, 1)
        qs.append(q)
        ps.append(p)
    return torch.stack(qs), torch.stack(ps)


def record_simulations(arrs):
    """Six steps of the lifted ``Simulator.simulate`` with the lifted ``VelocityVerlet`` and each hook on analytic float64 forces."""
    System = system_class()
    n_mol, m, p, q = base_system()
    N = int(n_mol.sum())
    env = {"torch": torch}
    half = _lift(_md_path("integrators.py"), "Integrator", ("half_step", "main_step"), env)
    main = _lift(_md_path("integrators.py"), "VelocityVerlet", ("_main_step",), env)
    simulate = _lift(_md_path("simulator.py"), "Simulator", ("simulate",), {"torch": torch, "nullcontext": nullcontext, "trange": None})["simulate"]
    noise = [langevin_noise(step, which, N_REPLICAS, N) for step in range(SIM_STEPS) for which in (0, 1)]
    hooks = {"nhc_global": lambda: hook_class("nhc")(T_BATH, TAU_FS, 3, False, 2, 3), "nhc_massive": lambda: hook_class("nhc")(T_BATH, TAU_FS, 3, True, 2, 3),
             "berendsen": lambda: hook_class("berendsen")(T_BATH, TAU_FS), "langevin": lambda: hook_class("langevin", noise)(T_BATH, TAU_FS)}
    for kind, make in hooks.items():
        th = make()
        events = []
        lifted_apply = type(th)._apply_thermostat
        type(th)._apply_thermostat = lambda self, simulator, la=lifted_apply: (events.append("thermostat"), la(self, simulator))[1]
        system = System(q.clone(), p.clone(), m, n_mol)
        traj_q, traj_p = [], []

        class Snapshot:
            def __getattr__(self, name):
                if not name.startswith("on_"):
                    raise AttributeError(name)
                return lambda simulator: None

            def on_step_finalize(self, simulator):
                traj_q.append(simulator.system.positions.clone())
                traj_p.append(simulator.system.momenta.clone())
        integ = types.SimpleNamespace(time_step=DT)
        integ._main_step = lambda s: (events.append("main_step"), main["_main_step"](integ, s))[1]
        integ.main_step = lambda s: half["main_step"](integ, s)
        integ.half_step = lambda s: (events.append("half_step"), half["half_step"](integ, s))[1]

        def calculate(s):
            events.append("calculate")
            s.forces = spring_forces(s.positions, s.index_m)
        sim = types.SimpleNamespace(system=system, integrator=integ, calculator=types.SimpleNamespace(calculate=calculate),
                                    simulator_hooks=[th, Snapshot()], step=0, effective_steps=0, n_steps=None, progress=False,
                                    gradients_required=False, device=torch.device("cpu"), dtype=torch.float64)
        simulate(sim, SIM_STEPS)
        assert sim.step == SIM_STEPS and len(traj_q) == SIM_STEPS
        q_ref, p_ref = torch.stack(traj_q), torch.stack(traj_p)
        per_step = (len(events) - 1) // SIM_STEPS
        assert events[1:1 + per_step] == ["thermostat", "half_step", "main_step", "calculate", "half_step", "thermostat"], events[:8]
        t = "sim_%s_" % kind
        arrs.update({t + "q": q_ref.numpy(), t + "p": p_ref.numpy(), t + "events": np.array(events[:1 + per_step])})
        if kind.startswith("nhc"):
            consts = {"kT": float(th.kb_temperature), "frequency": float(th.frequency), "steps": th.time_step.double(),
                      "m": th.masses.double().squeeze(2) if kind == "nhc_global" else th.masses.double()}
        elif kind == "berendsen":
            consts = {"tau": float(th.time_constant)}
        else:
            consts = {"c1": float(th.c1.reshape(-1)[0]), "c2": float(th.c2.reshape(-1)[0])}
        qo, po = oracle_trajectory(kind, "reference", consts)
        assert float((qo - q_ref).abs().max() / q_ref.abs().max()) < 1e-12 and float((po - p_ref).abs().max() / p_ref.abs().max()) < 1e-12, kind
        qw, pw = oracle_trajectory(kind, "after_half_step", consts)
        dq, dp = float((qw[-1] - q_ref[-1]).abs().max() / q_ref[-1].abs().max()), float((pw[-1] - p_ref[-1]).abs().max() / p_ref[-1].abs().max())
        print("  %-12s wrong order (thermostat after the half step), end state: positions %.3e momenta %.3e" % (kind, dq, dp))
        arrs.update({t + "wrong_q": qw[-1].numpy(), t + "wrong_p": pw[-1].numpy()})


def arrays():
    u = _md_units()
    arrs = {"unit_kB": u.kB, "unit_fs": u.fs, "temperature_bath": T_BATH, "temperature_start": T_START, "dt": DT, "tau_fs": TAU_FS,
            "applications": np.array(APPLICATIONS), "seed": np.uint64(SEED), "n_replicas": N_REPLICAS, "sim_steps": SIM_STEPS,
            "spring_k": SPRING_K, "spring_r0": SPRING_R0,
            "nhc_cases": np.array([c[0] for c in NHC_CASES]), "nhc_params": np.array([[c[1], c[2], c[3], int(c[4])] for c in NHC_CASES])}
    record_system(arrs)
    record_nhc(arrs)
    record_berendsen(arrs)
    record_langevin(arrs)
    record_simulations(arrs)
    return arrs


if __name__ == "__main__":
    a = arrays()
    save_npz_reproducible(OUT, a)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(a), os.path.getsize(OUT)))
