"""Generator of tests/golden/md_rp_thermostat.npz (a plain script, not collected by pytest):

    python tests/make_md_rp_thermostat_golden.py

It lifts, with ``ast`` at run time, the reference's own ``NHCRingPolymerThermostat`` (``_init_masses``, ``_compute_kinetic_energy``,
``_apply_thermostat`` over the lifted ``NHCThermostat._init_thermostat`` / ``_propagate_thermostat``), ``PILEGlobalThermostat.
_apply_thermostat`` and ``PILELocalThermostat`` (for TRPMD: ``thermostat_centroid=False`` and a damping factor, what
``TRPMDThermostat.__init__`` passes on) together with ``System.sum_atoms`` / ``expand_atoms``, the ``NormalModeTransformer`` and
``RingPolymer._init_propagator``, and stores ONLY the arrays they compute.  Every case runs on a float64 and on a float32 system:
the difference is the reference's own float32 gap, the yardstick of the device tolerances.

Size.  The file is kept to a few tens of kilobytes by storing nothing twice:
  * of a float32 run only what the tolerance rule reads, max |float32 - float64| per compared array (``nhc_gaps``, ``pile_gaps``);
  * start momenta and masses once per bead count (``p_b<B>`` / ``m_b<B>``: every thermostat starts from the same system);
  * the chain state of a ``local=False`` run as what distinguishes it from the ``local=True`` run of the same case: the chains of
    the modes k >= 1 are the same numbers (asserted here: to 1e-13 relative, the rounding of the momenta they are fed) and the
    centroid rows are one chain per molecule, broadcast over its atoms and components (asserted bit for bit), so ``nhc_<tag>_glo_f64_{v,f}c_<k>`` [n_molecules, chain_length] holds them;
  * constants that do not depend on ``local`` once per case, and the results of one run after 1, 2 and 6 applications as ONE array.

The integrator handed to ``NHCRingPolymerThermostat`` carries a COPY of ``omega_normal``: the reference overwrites its entry 0.

PILE-G: the noise is ``oracle.md_oracle.pile_noise`` of the batch, and the reference runs PER MOLECULE on its slice of that noise,
so that its ``thermostat_noise_centroid[0, 0, 0]`` is the molecule's own first atom (the project's rule for a batch); the case
``pgs_`` is ONE molecule of all atoms through the reference unsliced.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import md_oracle as MDO  # noqa: E402
from oracle.make_golden import _TorchWithNoise, _lift, _lifted_ring_polymer, _md_path, _md_units, _nm_transformer, save_npz_reproducible  # noqa: E402
import make_md_thermostat_golden as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "md_rp_thermostat.npz")

N_ATOMS_MOL = [2, 5, 9]
T_BATH, T_START = 300.0, 600.0
DT = 5.0e-4                      # 0.5 fs in ps
TAU_FS = 10.0
APPLICATIONS = (1, 2, 6)
STATE_AT = (1, 6)                # chain state stored after these applications
# (tag, n_beads, chain_length, multi_step, integration_order): three chain set-ups (one of length 1), one per bead count; each local and global
NHC_CASES = [("b1_l3_m2_o3", 1, 3, 2, 3), ("b3_l2_m4_o5", 3, 2, 4, 5), ("b4_l1_m1_o3", 4, 1, 1, 3)]
PILE_BEADS = (1, 3, 4)
TRPMD_BEADS = (3, 4)
TRPMD_DAMPING = 0.5
SEED = 0xC0FFEE123


def system_class():
    Base = G.system_class()

    def __init__(self, p, m, n_atoms_mol):
        Base.__init__(self, None, p, m, n_atoms_mol)
        self.nm_transform = _nm_transformer()(int(p.shape[0])).to(p.dtype)
    return type("LiftedRingSystem", (Base,), {
        "__init__": __init__,
        "momenta_normal": property(lambda s: s.nm_transform.beads2normal(s.momenta), lambda s, v: setattr(s, "momenta", s.nm_transform.normal2beads(v)))})


def base_system(n_beads, n_atoms_mol=N_ATOMS_MOL):
    from schnetpack_amd import md as MD
    n_mol = torch.tensor(n_atoms_mol)
    N = int(n_mol.sum())
    g = torch.Generator().manual_seed(177 + n_beads)
    m = torch.rand(1, N, 1, generator=g, dtype=torch.float64) * 15 + 1
    m[0, 0, 0], m[0, 1, 0] = 1.008, 200.0
    p = torch.randn(n_beads, N, 3, generator=g, dtype=torch.float64) * (m * MD.KB_MD * n_beads * T_START).sqrt()
    return n_mol, m, p


def integrator_for(n_beads, dtype):
    from schnetpack_amd import md as MD
    omega = MD.KB_MD * n_beads * T_BATH / MD.HBAR_MD
    integ = _lifted_ring_polymer(n_beads, omega, DT)
    return types.SimpleNamespace(time_step=DT, omega_normal=integ.omega_normal.to(dtype).clone(), omega=omega), integ.omega_normal.clone()


def nhc_rp_class():
    units = _md_units()
    env = {"torch": torch, "spk_units": units, "YSWeights": G.ys_weights_class()}
    fns = _lift(_md_path("simulation_hooks", "basic_hooks.py"), "SimulationHook",
                ("on_step_begin", "on_step_middle", "on_step_end", "on_step_finalize", "on_simulation_start", "on_simulation_end"), env)
    fns.update(_lift(_md_path("simulation_hooks", "thermostats.py"), "ThermostatHook", ("on_simulation_start", "on_step_begin", "on_step_end"), env))
    fns.update(_lift(_md_path("simulation_hooks", "thermostats.py"), "NHCThermostat", ("_init_thermostat", "_propagate_thermostat"), env))
    fns.update(_lift(_md_path("simulation_hooks", "thermostats_rpmd.py"), "NHCRingPolymerThermostat", ("_init_masses", "_compute_kinetic_energy", "_apply_thermostat"), env))

    def __init__(self, temperature_bath, time_constant, local, chain_length, multi_step, integration_order):
        # buffers of ThermostatHook / NHCThermostat / NHCRingPolymerThermostat.__init__ (massive=True)
        self.temperature_bath = torch.tensor(temperature_bath)
        self.time_constant = torch.tensor(time_constant * units.fs)
        self.initialized = False
        self.chain_length, self.massive, self.local = torch.tensor(chain_length), torch.tensor(True), torch.tensor(local)
        self.frequency = 1.0 / self.time_constant
        self.kb_temperature = self.temperature_bath * units.kB
        self.multi_step, self.integration_order = torch.tensor(multi_step), torch.tensor(integration_order)
    fns["__init__"] = __init__
    fns["to"] = G._to
    return type("LiftedNHCRingPolymerThermostat", (), fns)


def pile_class(kind, noise):
    units = _md_units()
    env = {"torch": _TorchWithNoise(noise), "spk_units": units}
    fns = _lift(_md_path("simulation_hooks", "basic_hooks.py"), "SimulationHook",
                ("on_step_begin", "on_step_middle", "on_step_end", "on_step_finalize", "on_simulation_start", "on_simulation_end"), env)
    fns.update(_lift(_md_path("simulation_hooks", "thermostats.py"), "ThermostatHook", ("on_simulation_start", "on_step_begin", "on_step_end"), env))
    fns.update(_lift(_md_path("simulation_hooks", "thermostats_rpmd.py"), "PILELocalThermostat", ("_init_thermostat", "_apply_thermostat"), env))
    if kind == "global":
        fns.update(_lift(_md_path("simulation_hooks", "thermostats_rpmd.py"), "PILEGlobalThermostat", ("_apply_thermostat",), env))

    def __init__(self, temperature_bath, time_constant, thermostat_centroid=True, damping_factor=1.0):
        self.temperature_bath = torch.tensor(temperature_bath)
        self.time_constant = torch.tensor(time_constant * units.fs)
        self.thermostat_centroid, self.damping_factor = torch.tensor(thermostat_centroid), torch.tensor(damping_factor)
        self.initialized = False
    fns["__init__"] = __init__
    fns["to"] = G._to          # the registered buffers follow the dtype of the simulator (nn.Module.to); c1 / c2 are made afterwards
    return type("LiftedPILE_" + kind, (), fns)


def gap(r32, r64):
    return float((r32.double() - r64).abs().max())


def record_nhc(arrs):
    System = system_class()
    first = (torch.cumsum(torch.tensor(N_ATOMS_MOL), 0) - torch.tensor(N_ATOMS_MOL))
    idx_m = torch.repeat_interleave(torch.arange(len(N_ATOMS_MOL)), torch.tensor(N_ATOMS_MOL))
    # [case, local / global, p / v / f, application]; NaN where nothing is compared (chain state after 2 applications)
    gaps = np.full((len(NHC_CASES), 2, 3, len(APPLICATIONS)), np.nan)
    for ci, (tag, B, L, ms, order) in enumerate(NHC_CASES):
        n_mol, m, p = base_system(B)
        res = {}
        for local in (True, False):
            name = "nhc_%s_%s" % (tag, "loc" if local else "glo")
            for dt_tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
                th = nhc_rp_class()(T_BATH, TAU_FS, local, L, ms, order)
                system = System(p.to(dtype).clone(), m.to(dtype), n_mol)
                integ, omega_normal = integrator_for(B, dtype)
                sim = types.SimpleNamespace(system=system, integrator=integ, device=torch.device("cpu"), dtype=dtype)
                th.on_simulation_start(sim)
                assert th.velocities.dtype == dtype and th.masses.dtype == dtype and tuple(th.velocities.shape) == (B, 16, 3, L)
                if dt_tag == "f64":
                    arrs[name + "_masses"] = th.masses[:, :, 0, :].numpy().copy()
                    if local:
                        arrs["nhc_%s_consts" % tag] = np.array([float(th.kb_temperature), float(th.frequency), float(integ.omega)])   # kT, frequency, omega
                        arrs["nhc_%s_steps" % tag] = th.time_step.numpy().copy()
                        arrs["nhc_%s_omega_normal" % tag] = omega_normal.numpy().copy()
                for k in range(1, max(APPLICATIONS) + 1):
                    th.on_step_begin(sim)
                    assert system.momenta.dtype == dtype
                    if k in APPLICATIONS:
                        res[local, dt_tag, "p", k] = system.momenta.clone()
                    if k in STATE_AT:
                        res[local, dt_tag, "v", k], res[local, dt_tag, "f", k] = th.velocities.clone(), th.forces.clone()
        kept = {}
        for (local, dt_tag, key, k), t in res.items():
            name = "nhc_%s_%s" % (tag, "loc" if local else "glo")
            if dt_tag == "f32":
                gaps[ci, 0 if local else 1, "pvf".index(key), APPLICATIONS.index(k)] = gap(t, res[local, "f64", key, k])
            elif key == "p" or local:
                kept.setdefault("%s_f64_%s" % (name, key), []).append(t)
            else:
                loc = res[True, "f64", key, k]
                # the chains of the modes k >= 1 do not see the centroid; what differs is the rounding of the back-transformed momenta they
                # are fed after the first application (seen: 1e-15 relative; the tests compare at 1e-12 and at float32 ulps)
                assert B == 1 or float((t[1:] - loc[1:]).abs().max()) <= 1e-13 * float(loc[1:].abs().max())
                mol = t[0, first, 0, :]                                                # [n_molecules, L]
                assert torch.equal(t[0], mol[idx_m][:, None, :].expand(16, 3, L))      # one centroid chain per molecule
                kept.setdefault("%s_f64_%sc" % (name, key), []).append(mol)
        # one array per quantity, first axis = the applications it was taken after (APPLICATIONS for p, STATE_AT for the chain state)
        arrs.update({k: torch.stack(v).numpy().copy() for k, v in kept.items()})
    arrs["nhc_gaps"] = gaps


def run_pile(kind, B, p, m, n_mol, noise, dtype, **kw):
    """max(APPLICATIONS) applications of the lifted hook on one system; returns the momenta after each and (c1, c2)."""
    System = system_class()
    th = pile_class(kind, list(noise))(T_BATH, TAU_FS, **kw)
    system = System(p.to(dtype).clone(), m.to(dtype), n_mol)
    integ, _ = integrator_for(B, torch.float32)          # omega_normal is a float32 buffer: PILE coefficients are float32
    sim = types.SimpleNamespace(system=system, integrator=integ, device=None, dtype=dtype)
    th.on_simulation_start(sim)
    out = []
    for k in range(max(APPLICATIONS)):
        th.on_step_begin(sim)
        out.append(system.momenta.clone())
    return out, th.c1.reshape(-1).double(), th.c2.reshape(-1).double()


PILE_CASES = ["pg_b%d" % B for B in PILE_BEADS] + ["pgs"] + ["tr_b%d" % B for B in TRPMD_BEADS]


def record_pile(arrs):
    n_apps = max(APPLICATIONS)
    gaps = np.zeros((len(PILE_CASES), len(APPLICATIONS)))          # max |float32 run - float64 run| of the reference, per case and application

    def keep(case, o64, o32):
        arrs["%s_f64_p" % case] = torch.stack([o64[k - 1] for k in APPLICATIONS]).numpy().copy()          # first axis: APPLICATIONS
        for i, k in enumerate(APPLICATIONS):
            gaps[PILE_CASES.index(case), i] = gap(o32[k - 1], o64[k - 1])
    for B in PILE_BEADS:
        n_mol, m, p = base_system(B)
        N = int(n_mol.sum())
        noise = [MDO.pile_noise(B, N, SEED, step, 0) for step in range(n_apps)]
        first = (torch.cumsum(n_mol, 0) - n_mol).tolist()
        outs = {}
        for dt_tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            outs[dt_tag] = [torch.zeros(B, N, 3, dtype=dtype) for _ in range(n_apps)]
            for a0, na in zip(first, n_mol.tolist()):       # the reference per molecule, on its slice of the batch noise
                sl = slice(a0, a0 + na)
                o, c1, c2 = run_pile("global", B, p[:, sl], m[:, sl], torch.tensor([na]), [x[:, sl] for x in noise], dtype)
                for k in range(n_apps):
                    outs[dt_tag][k][:, sl] = o[k]
        keep("pg_b%d" % B, outs["f64"], outs["f32"])
        arrs["pg_b%d_c12" % B] = torch.stack([c1, c2]).numpy()
    # one molecule of all atoms, unsliced
    B = 3
    n_mol, m, p = base_system(B, [16])
    assert torch.equal(p, base_system(B)[2])                # the same start as the batch of three: stored once, as p_b3
    noise = [MDO.pile_noise(B, 16, SEED, step, 0) for step in range(n_apps)]
    arrs["pgs_n_beads"] = B
    o64, c1, c2 = run_pile("global", B, p, m, n_mol, noise, torch.float64)
    keep("pgs", o64, run_pile("global", B, p, m, n_mol, noise, torch.float32)[0])
    arrs["pgs_c12"] = torch.stack([c1, c2]).numpy()
    for B in TRPMD_BEADS:
        n_mol, m, p = base_system(B)
        noise = [MDO.pile_noise(B, 16, SEED, step, 0) for step in range(n_apps)]
        # TRPMDThermostat.__init__ (thermostats_rpmd.py:228-234): time_constant 1.0, no centroid thermostat, the damping factor
        kw = dict(thermostat_centroid=False, damping_factor=TRPMD_DAMPING)
        o64, c1, c2 = run_pile("local", B, p, m, n_mol, noise, torch.float64, **kw)
        keep("tr_b%d" % B, o64, run_pile("local", B, p, m, n_mol, noise, torch.float32, **kw)[0])
        arrs["tr_b%d_c12" % B] = torch.stack([c1, c2]).numpy()
    arrs["pile_gaps"] = gaps


def arrays():
    u = _md_units()
    n_mol = torch.tensor(N_ATOMS_MOL)
    arrs = {"unit_kB": u.kB, "unit_fs": u.fs, "unit_hbar": u.hbar, "temperature_bath": T_BATH, "temperature_start": T_START, "dt": DT,
            "tau_fs": TAU_FS, "applications": np.array(APPLICATIONS), "state_at": np.array(STATE_AT), "seed": np.uint64(SEED),
            "n_atoms": n_mol.numpy(), "idx_m": torch.repeat_interleave(torch.arange(3), n_mol).numpy(),
            "nhc_cases": np.array([c[0] for c in NHC_CASES]), "nhc_params": np.array([list(c[1:]) for c in NHC_CASES]),
            "pile_beads": np.array(PILE_BEADS), "trpmd_beads": np.array(TRPMD_BEADS), "trpmd_damping": TRPMD_DAMPING}
    for B in sorted(set(PILE_BEADS) | set(TRPMD_BEADS) | {c[1] for c in NHC_CASES}):
        _, m, p = base_system(B)
        arrs.update({"p_b%d" % B: p.numpy(), "m_b%d" % B: m.numpy()})
    arrs["pile_cases"] = np.array(PILE_CASES)
    record_nhc(arrs)
    record_pile(arrs)
    return arrs


if __name__ == "__main__":
    a = arrays()
    save_npz_reproducible(OUT, a)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(a), os.path.getsize(OUT)))
