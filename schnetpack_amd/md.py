"""MD steps around the force call: the velocity-Verlet and ring-polymer
integrators of the reference (md/integrators.py:24-229) on fused HIP kernels, and a bead-parallel ring
polymer (one bead per rank, one all-gather per step).  Unit agnostic: ``time_step`` is in the unit system
of the tensors handed in (the reference's MD internal units are kJ/mol, nm, Dalton => ps; 1 fs = 1e-3).

``state`` objects only need ``positions``, ``momenta``, ``forces`` ([n_replicas, n_atoms, 3]) and
``masses`` ([1, n_atoms, 1] or [n_atoms]) attributes -- what ``schnetpack.md.System`` has.
"""
import math
import os
import struct
from typing import Optional

import torch

from . import _lib
from ._lib import check, fptr, lib, stream

__all__ = ["BerendsenThermostat", "LangevinThermostat", "NHCThermostat", "NVTSimulation", "nhc_sub_steps", "langevin_coefficients", "YS_WEIGHTS",
           "PILELocalThermostat", "PILEGlobalThermostat", "TRPMDThermostat", "NHCRingPolymerThermostat", "rp_nhc_frequencies", "pile_coefficients", "pile_matrices", "VelocityVerlet", "RingPolymer", "NVESimulation", "RPMDSimulation", "MDState", "fold_replicas", "normal_mode_matrix", "ring_polymer_propagator", "ring_polymer_matrices",
           "KB_MD", "HBAR_MD", "FS_MD"]

# reference MD internal units (kJ/mol, nm, Dalton): time unit = 1 ps (units.py:10-40)
FS_MD = 1.0e-3
KB_MD = 8.314462618e-3          # kJ / (mol K)
HBAR_MD = 6.350779923e-2        # kJ / mol * ps


def _flat_masses(masses: torch.Tensor, n_atoms: int) -> torch.Tensor:
    m = masses.reshape(-1)
    if m.numel() != n_atoms:
        raise _lib.SpkHipError("masses: expected %d entries, got %d" % (n_atoms, m.numel()))
    return m.float().contiguous()


class VelocityVerlet:
    """md/integrators.py:24-110.  ``half_step`` / ``main_step`` as in the reference, plus
    ``first_half_and_main_step`` which fuses the two that are adjacent in the MD loop
    (md/simulator.py:126-150) into one pass and evaluates the neighbour-list skin criterion on the way."""

    ring_polymer = False
    pressure_control = False

    def __init__(self, time_step: float):
        self.time_step = float(time_step)

    def half_step(self, state):
        p = state.momenta
        with torch.cuda.device(p.device):
            check(lib().spk_md_half_step_f32(fptr(p), fptr(state.forces.contiguous()), 0.5 * self.time_step, p.numel(), stream()))

    def main_step(self, state):
        self.first_half_and_main_step(state, kick=False)

    def first_half_and_main_step(self, state, kick: bool = True, reference_positions: Optional[torch.Tensor] = None,
                                 max_displacement: float = 0.0, flag: Optional[torch.Tensor] = None):
        R, p = state.positions, state.momenta
        n_rep = R.shape[0] if R.dim() == 3 else 1
        n_atoms = R.numel() // 3
        m = _flat_masses(state.masses, n_atoms // n_rep)
        if n_rep > 1:
            m = m.repeat(n_rep)
        F = state.forces.contiguous() if kick else None
        with torch.cuda.device(R.device):
            check(lib().spk_md_kick_drift_f32(fptr(R), fptr(p), fptr(F), fptr(m), self.time_step, n_atoms,
                                              fptr(reference_positions), float(max_displacement) ** 2,
                                              _lib.iptr(flag, torch.int32) if flag is not None else None, stream()))


def normal_mode_matrix(n_beads: int) -> torch.Tensor:
    """C[k, n] (md/utils/normal_model_transformation.py:38-68), float64."""
    B = n_beads
    n = torch.arange(1, B + 1, dtype=torch.float64)
    C = torch.zeros(B, B, dtype=torch.float64)
    C[0] = 1.0
    for k in range(1, B // 2 + 1):
        C[k] = math.sqrt(2.0) * torch.cos(2.0 * math.pi * k * n / B)
    for k in range(B // 2 + 1, B):
        C[k] = math.sqrt(2.0) * torch.sin(2.0 * math.pi * k * n / B)
    if B % 2 == 0:
        C[B // 2] = torch.where(n.long() % 2 == 0, 1.0, -1.0).double()
    return C / math.sqrt(B)


def ring_polymer_propagator(n_beads: int, omega: float, time_step: float) -> torch.Tensor:
    """[n_beads, 2, 2] free ring-polymer propagator in normal modes (md/integrators.py:152-199)."""
    on = 2.0 * omega * torch.sin(torch.arange(n_beads).float() * math.pi / n_beads)
    odt = on * time_step
    P = torch.zeros(n_beads, 2, 2)
    P[:, 0, 0] = torch.cos(odt)
    P[:, 1, 1] = torch.cos(odt)
    P[:, 0, 1] = -torch.sin(odt) * on
    P[1:, 1, 0] = torch.sin(odt)[1:] / on[1:]
    P[0, 1, 0] = time_step
    return P


def ring_polymer_matrices(n_beads: int, omega: float, time_step: float) -> torch.Tensor:
    """A [4, B, B] = C^T diag(P_ij) C for (ij) = pp, pq, qp, qq: transform, propagate and back-transform
    folded into bead-space matrices (they are linear maps; evaluated in float64, stored float32)."""
    C = normal_mode_matrix(n_beads)
    P = ring_polymer_propagator(n_beads, omega, time_step).double()
    return torch.stack([C.t() @ torch.diag(P[:, i, j]) @ C for (i, j) in ((0, 0), (0, 1), (1, 0), (1, 1))]).float().contiguous()


class RingPolymer(VelocityVerlet):
    """md/integrators.py:113-229.  ``positions`` / ``momenta`` are [n_beads, n_atoms, 3].

    Single process: all beads local.  Bead-parallel (``group`` given, one contiguous bead chunk per rank,
    SURVEY.md section 8(e)): the rank's [n_local, n_atoms, 3] positions and momenta are packed into one
    buffer, all-gathered ONCE per step (RCCL over xGMI; 2 x 384 KB per rank at 32 k atoms) and every
    rank evaluates only its own beads of the mixed result -- no second exchange for the back-transform.
    """

    ring_polymer = True

    def __init__(self, time_step: float, n_beads: int, temperature: float, omega: Optional[float] = None,
                 group=None, compute_fn=None):
        super().__init__(time_step)
        self.n_beads = int(n_beads)
        self.omega = float(omega) if omega is not None else KB_MD * n_beads * temperature / HBAR_MD
        self.A = ring_polymer_matrices(self.n_beads, self.omega, self.time_step)
        self.group = group
        self._compute = compute_fn or _ring_polymer_hip
        self._A_dev = None

    def _bead_range(self):
        if self.group is None:
            return 0, self.n_beads, 1
        import torch.distributed as dist
        from .parallel import shard_frames
        world, rank = dist.get_world_size(self.group), dist.get_rank(self.group)
        lo, hi = shard_frames(self.n_beads, rank, world)
        if (hi - lo) * world != self.n_beads:
            raise ValueError("bead-parallel ring polymer needs n_beads divisible by the number of ranks")
        return lo, hi, world

    def main_step(self, state):
        q, p = state.positions, state.momenta
        lo, hi, world = self._bead_range()
        n_local = hi - lo
        if q.shape[0] != n_local:
            raise ValueError("expected %d local beads, got %d" % (n_local, q.shape[0]))
        n_atoms = q.shape[1]
        if self._A_dev is None or self._A_dev.device != q.device:
            self._A_dev = self.A.to(q.device)
        if world > 1:
            import torch.distributed as dist
            local = torch.stack([q, p]).contiguous()                      # [2, n_local, n, 3]
            allb = torch.empty(world * local.numel(), dtype=local.dtype, device=local.device)
            dist.all_gather_into_tensor(allb, local.view(-1), group=self.group)
            allb = allb.view((world,) + tuple(local.shape))                # [world, 2, n_local, n, 3]
            q_all = allb[:, 0].reshape(self.n_beads, n_atoms, 3).contiguous()
            p_all = allb[:, 1].reshape(self.n_beads, n_atoms, 3).contiguous()
        else:
            q_all, p_all = q.contiguous(), p.contiguous()
        q_new, p_new = self._compute(q_all, p_all, state.masses, self._A_dev, lo, n_local)
        state.positions, state.momenta = q_new, p_new


def _ring_polymer_hip(q_all, p_all, masses, A, bead0, n_local, q_out=None, p_out=None, reference_positions=None,
                      max_displacement=0.0, flag=None):
    B, n_atoms = int(q_all.shape[0]), int(q_all.shape[1])
    m = _flat_masses(masses, n_atoms).to(q_all.device)
    if q_out is None:
        q_out = torch.empty((n_local, n_atoms, 3), dtype=torch.float32, device=q_all.device)
        p_out = torch.empty_like(q_out)
    with torch.cuda.device(q_all.device):
        check(lib().spk_md_ring_polymer_step_f32(fptr(q_all), fptr(p_all), fptr(m), fptr(A), B, n_atoms, int(bead0), int(n_local),
                                                 fptr(q_out), fptr(p_out), fptr(reference_positions), float(max_displacement) ** 2,
                                                 _lib.iptr(flag, torch.int32) if flag is not None else None, stream()))
    return q_out, p_out


def pile_coefficients(n_beads: int, omega: float, time_step: float, time_constant: float, thermostat_centroid: bool = True,
                      damping_factor: float = 1.0):
    """(c1 [B], c2 [B]) of the PILE-L thermostat (md/simulation_hooks/thermostats_rpmd.py:66-92), float64: gamma_k = 2 omega_k
    (centroid: 1 / time_constant) x damping factor, c1 = exp(-dt/2 gamma), c2 = sqrt(1 - c1^2).  The reference evaluates this in
    float32, where 1 - c1^2 cancels; tests/golden/md_pile.npz holds its values and tests/test_md_reference.py the bound."""
    on = 2.0 * omega * torch.sin(torch.arange(n_beads).float() * math.pi / n_beads)
    gamma = 2.0 * on.double()
    if thermostat_centroid:
        gamma[0] = 1.0 / time_constant
    gamma = gamma * damping_factor
    c1 = torch.exp(-0.5 * time_step * gamma)
    return c1, torch.sqrt(1.0 - c1 ** 2)


def pile_matrices(n_beads: int, omega: float, time_step: float, time_constant: float, thermostat_centroid: bool = True,
                  damping_factor: float = 1.0) -> torch.Tensor:
    """M [2, B, B] = (C^T diag(c1) C, C^T diag(c2)) with the ``pile_coefficients``: the transform to normal modes, the scaling
    and the back-transform of the PILE-L thermostat folded into bead-space matrices (float64 -> float32)."""
    C = normal_mode_matrix(n_beads)
    c1, c2 = pile_coefficients(n_beads, omega, time_step, time_constant, thermostat_centroid, damping_factor)
    return torch.stack([C.t() @ torch.diag(c1) @ C, C.t() @ torch.diag(c2)]).float().contiguous()


def _pile_hip(p_all, masses, M, noise_scale, seed, step, step_dev, which, bead0, n_local, p_out=None):
    B, n_atoms = int(p_all.shape[0]), int(p_all.shape[1])
    m = _flat_masses(masses, n_atoms).to(p_all.device)
    if p_out is None:
        p_out = torch.empty((n_local, n_atoms, 3), dtype=torch.float32, device=p_all.device)
    with torch.cuda.device(p_all.device):
        check(lib().spk_md_pile_f32(fptr(p_all), fptr(m), fptr(M), float(noise_scale), int(seed), int(step),
                                    _lib.iptr(step_dev) if step_dev is not None else None, int(which), B, n_atoms, int(bead0), int(n_local),
                                    fptr(p_out), stream()))
    return p_out


def _apply_to_state(thermostat, state, step: int = 0, which: int = 0, step_dev=None, out=None):
    """``apply`` of every ring-polymer thermostat: the momenta of all beads (bead-parallel: ONE all-gather over ``thermostat.group``)
    go to ``thermostat.apply_beads``, which returns the thermostatted beads of this rank; they become ``state.momenta``."""
    p = state.momenta
    lo, hi, world = thermostat._range()
    if world > 1:
        import torch.distributed as dist
        local = p.contiguous()
        allb = torch.empty((world,) + tuple(local.shape), dtype=local.dtype, device=local.device)
        dist.all_gather_into_tensor(allb.view(-1), local.view(-1), group=thermostat.group)
        p_all = allb.reshape(thermostat.n_beads, p.shape[1], 3)
    else:
        p_all = p.contiguous()
    state.momenta = thermostat.apply_beads(p_all, state.masses, lo, hi - lo, step, step_dev, which, out)
    return state.momenta


class PILELocalThermostat:
    """Mirror of the reference's ``PILELocalThermostat`` (md/simulation_hooks/thermostats_rpmd.py:33-119; constructor
    arguments and the two application points of md/simulation_hooks/thermostats.py:97-123) for the device ring polymer:
    ``apply(state, step, which)`` replaces the momenta by ``C^T (c1 C p + sqrt(m kB n T) c2 xi)``.

    Bead-parallel (``group``): ONE all-gather of the momenta per application; the noise is a counter-based stream
    (Philox keyed by seed / step / atom / mode, ``spk_md_pile_f32``) that every rank regenerates identically, so there is
    no second exchange and the trajectory does not depend on the number of ranks.  ``step_dev`` (a device int64 word the
    caller increments inside its captured step) makes replays of a HIP graph draw fresh noise."""

    ring_polymer = True

    def __init__(self, temperature_bath: float, time_constant: float, thermostat_centroid: bool = True, damping_factor: float = 1.0,
                 seed: int = 0, group=None, compute_fn=None, fs: float = FS_MD, kb: float = KB_MD):
        # ``time_constant`` is in FEMTOSECONDS like the reference's (LangevinThermostat.__init__ multiplies by spk_units.fs,
        # md/simulation_hooks/thermostats.py); ``fs`` / ``kb`` are 1 fs and Boltzmann's constant in the unit system of the
        # state tensors (defaults: the reference's MD internal units kJ/mol, nm, Dalton => ps)
        self.temperature_bath, self.time_constant = float(temperature_bath), float(time_constant) * float(fs)
        self.kb = float(kb)
        self.thermostat_centroid, self.damping_factor = bool(thermostat_centroid), float(damping_factor)
        self.seed, self.group = int(seed), group
        self._compute = compute_fn or _pile_hip
        self.M = None
        self._M_dev = None

    def init(self, integrator: RingPolymer, idx_m: Optional[torch.Tensor] = None, n_atoms: Optional[torch.Tensor] = None):
        """``_init_thermostat``: coefficients from the normal-mode frequencies of the integrator.  The molecule layout is accepted
        for the common signature of the ring-polymer thermostats; PILE-L couples nothing across atoms and does not use it."""
        self.n_beads = integrator.n_beads
        self.M = self._matrices(integrator)
        self.noise_scale = math.sqrt(self.kb * self.n_beads * self.temperature_bath)
        self._range = integrator._bead_range if self.group is None else RingPolymer(integrator.time_step, self.n_beads, 1.0, omega=1.0,
                                                                                    group=self.group)._bead_range
        return self

    def _matrices(self, integrator):
        return pile_matrices(self.n_beads, integrator.omega, integrator.time_step, self.time_constant, self.thermostat_centroid,
                             self.damping_factor)

    def apply(self, state, step: int = 0, which: int = 0, step_dev=None, out=None):
        return _apply_to_state(self, state, step, which, step_dev, out)

    def apply_beads(self, p_all, masses, bead0, n_local, step=0, step_dev=None, which=0, out=None):
        """The one entry ``RPMDSimulation`` calls for every ring-polymer thermostat: the momenta of ALL beads [n_beads, n_atoms, 3]
        in, the thermostatted beads [bead0, bead0 + n_local) out (``out`` or a new tensor; never ``p_all``)."""
        if self._M_dev is None or self._M_dev.device != p_all.device:
            self._M_dev = self.M.to(p_all.device)
        return self._compute(p_all, masses, self._M_dev, self.noise_scale, self.seed, step, step_dev, which, bead0, n_local, out)

    def prepare(self, p_all, masses):
        """Device buffers before a graph capture; PILE-L owns only its matrices."""
        if self._M_dev is None or self._M_dev.device != p_all.device:
            self._M_dev = self.M.to(p_all.device)

    def state_dict(self):
        return {}

    def load_state_dict(self, sd):
        pass


# ------------------------------------------------------------------------------------------------ classical NVT thermostats
# Yoshida-Suzuki weights of the chain integrator (md/utils/thermostat_utils.py:18-44; Yoshida, Phys. Lett. A 150 (1990) 262).  The
# reference has no entry for order 1; the trivial weight [1] is what a single unsplit sub-step is.
YS_WEIGHTS = {
    1: (1.0,),
    3: (1.35120719195966, -1.70241438391932, 1.35120719195966),
    5: (0.41449077179438, 0.41449077179438, -0.65796308717750, 0.41449077179438, 0.41449077179438),
    7: (0.78451361047756, 0.23557321335936, -1.17767998417887, 1.31518632068390, -1.17767998417887, 0.23557321335936, 0.78451361047756),
}


def nhc_sub_steps(time_step: float, multi_step: int = 2, integration_order: int = 3):
    """``time_step * w_k / multi_step`` (thermostats.py:332-341), float64 list of ``integration_order`` entries."""
    if integration_order not in YS_WEIGHTS:
        raise ValueError("Order %d not supported for YS integration weights (1, 3, 5, 7)" % integration_order)
    if multi_step < 1:
        raise ValueError("multi_step must be at least 1")
    return [float(time_step) * w / int(multi_step) for w in YS_WEIGHTS[integration_order]]


class _ThermostatHip:
    """The device side of the classical thermostats (csrc/spk_md_thermo.hip through the C ABI).  A ``compute_fn`` handed to a
    thermostat is an object with these methods (tests/md_thermostat_oracle.py has a float64 host stand-in); every method works in
    place on buffers the thermostat owns, so a captured graph replays it."""

    @staticmethod
    def workspace(n_rep, n_atoms, n_mol, device):
        nbytes = int(lib().spk_md_kinetic_workspace_bytes(n_rep, n_atoms, n_mol))
        if nbytes < 0:
            raise _lib.SpkHipError("spk_md_kinetic_workspace_bytes: bad sizes")
        return torch.empty(max(nbytes, 4) // 4, dtype=torch.int32, device=device)

    @staticmethod
    def kinetic(p, masses, idx_m, n_mol, ke2, err, ws):
        n_rep, n_atoms = int(p.shape[0]), int(p.shape[1])
        with torch.cuda.device(p.device):
            check(lib().spk_md_kinetic_f32(fptr(p), fptr(masses), _lib.iptr(idx_m), n_rep, n_atoms, int(n_mol), fptr(ke2),
                                           _lib.iptr(err, torch.int32), _lib.iptr(ws, torch.int32), stream()))

    @staticmethod
    def _steps(sub_steps):
        import ctypes
        return (ctypes.c_float * len(sub_steps))(*sub_steps)

    @classmethod
    def nhc_global(cls, ke2, n_atoms_mol, n_rep, chain_length, multi_step, order, sub_steps, kT, link_mass, vel, frc, scale):
        with torch.cuda.device(ke2.device):
            check(lib().spk_md_nhc_global_f32(fptr(ke2), _lib.iptr(n_atoms_mol), int(n_rep), int(n_atoms_mol.shape[0]), int(chain_length),
                                              int(multi_step), int(order), cls._steps(sub_steps), float(kT), float(link_mass), fptr(vel),
                                              fptr(frc), fptr(scale), stream()))

    @classmethod
    def nhc_massive(cls, p, masses, chain_length, multi_step, order, sub_steps, kT, link_mass, vel, frc):
        with torch.cuda.device(p.device):
            check(lib().spk_md_nhc_massive_f32(fptr(p), fptr(masses), int(p.shape[0]), int(p.shape[1]), int(chain_length), int(multi_step),
                                               int(order), cls._steps(sub_steps), float(kT), float(link_mass), fptr(vel), fptr(frc), stream()))

    @staticmethod
    def berendsen_scale(ke2, n_atoms_mol, n_rep, dt_over_tau, temperature_bath, kb, scale):
        with torch.cuda.device(ke2.device):
            check(lib().spk_md_berendsen_scale_f32(fptr(ke2), _lib.iptr(n_atoms_mol), int(n_rep), int(n_atoms_mol.shape[0]), float(dt_over_tau),
                                                   float(temperature_bath), float(kb), fptr(scale), stream()))

    @staticmethod
    def scale_molecules(p, scale, idx_m, n_mol, err):
        with torch.cuda.device(p.device):
            check(lib().spk_md_scale_molecules_f32(fptr(p), fptr(scale), _lib.iptr(idx_m), int(p.shape[0]), int(p.shape[1]), int(n_mol),
                                                   _lib.iptr(err, torch.int32), stream()))


class _ClassicalThermostat:
    """What the three classical thermostats share (``ThermostatHook``, thermostats.py:41-146): bath temperature, time constant in fs,
    the molecule layout of the batch and the per-molecule kinetic reduction.  ``fs`` / ``kb`` as in ``PILELocalThermostat``."""

    ring_polymer = False

    def __init__(self, temperature_bath: float, time_constant: float, compute_fn=None, fs: float = FS_MD, kb: float = KB_MD):
        self.temperature_bath, self.time_constant = float(temperature_bath), float(time_constant) * float(fs)
        self.kb = float(kb)
        self._compute = compute_fn or self._default_compute()
        self.time_step = None
        self._idx_m = self._n_atoms_mol = None
        self._ready = None

    @staticmethod
    def _default_compute():
        return _ThermostatHip

    def init(self, simulation_or_integrator, idx_m: Optional[torch.Tensor] = None, n_atoms: Optional[torch.Tensor] = None):
        """``on_simulation_start``: the time step of the integrator and the molecule layout -- ``idx_m`` / ``n_atoms`` given, or
        those of a simulation's batch (``inputs``), or ONE molecule of all atoms."""
        sim = simulation_or_integrator
        integrator = getattr(sim, "integrator", sim)
        if getattr(integrator, "ring_polymer", False):
            raise ValueError("%s is a classical thermostat (ring_polymer = False): ring-polymer states keep PILELocalThermostat through "
                             "RPMDSimulation" % type(self).__name__)
        self.time_step = float(integrator.time_step)
        inputs = getattr(sim, "inputs", None)
        if idx_m is None and inputs is not None:
            from . import properties as P
            idx_m, n_atoms = inputs[P.idx_m], inputs[P.n_atoms]
        if idx_m is not None:
            idx_m, n_atoms = idx_m.long().contiguous(), n_atoms.long().contiguous()
            if idx_m.numel() > 1 and bool((idx_m[1:] < idx_m[:-1]).any()):
                raise ValueError("idx_m must ascend (atoms of a molecule contiguous)")
            if idx_m.numel() and (int(idx_m.min()) < 0 or int(idx_m.max()) >= int(n_atoms.shape[0])):
                raise ValueError("idx_m outside [0, n_molecules)")
        self._idx_m, self._n_atoms_mol = idx_m, n_atoms
        self._ready = None
        self._init_thermostat()
        return self

    def _init_thermostat(self):
        pass

    def _prepare(self, state):
        """Buffers on the device of the state, allocated once (before any graph capture: ``NVTSimulation`` calls this at set-up)."""
        p = state.momenta
        key = (p.device, p.dtype, tuple(p.shape))
        if self._ready == key:
            return
        if self.time_step is None:
            raise RuntimeError("%s.init(simulation_or_integrator) has not been called" % type(self).__name__)
        if p.dim() != 3 or p.shape[2] != 3:
            raise ValueError("momenta must be [n_replicas, n_atoms, 3]")
        n_rep, N = int(p.shape[0]), int(p.shape[1])
        dev = p.device
        if self._idx_m is None:
            self._idx_m, self._n_atoms_mol = torch.zeros(N, dtype=torch.long), torch.tensor([N], dtype=torch.long)
        if int(self._idx_m.shape[0]) != N:
            raise ValueError("idx_m has %d entries for %d atoms" % (int(self._idx_m.shape[0]), N))
        self._idx_m, self._n_atoms_mol = self._idx_m.to(dev), self._n_atoms_mol.to(dev)
        self.n_replicas, self.n_atoms, self.n_molecules = n_rep, N, int(self._n_atoms_mol.shape[0])
        self._masses = state.masses.reshape(-1).to(dev, p.dtype).contiguous()
        if self._masses.numel() != N:
            raise ValueError("masses: expected %d entries, got %d" % (N, self._masses.numel()))
        self._ke2 = torch.zeros(n_rep * self.n_molecules, dtype=p.dtype, device=dev)
        self._scale = torch.ones(n_rep * self.n_molecules, dtype=p.dtype, device=dev)
        self._err = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ws = self._compute.workspace(n_rep, N, self.n_molecules, dev)
        self._prepare_thermostat(p)
        self._ready = key

    def _prepare_thermostat(self, p):
        pass

    def _momenta(self, state):
        p = state.momenta
        if not p.is_contiguous():
            raise ValueError("momenta must be contiguous (they are updated in place)")
        self._prepare(state)
        return p

    def kinetic_energy2(self, state) -> torch.Tensor:
        """``2 E_kin`` per replica and molecule, [n_replicas, n_molecules] (a view of the thermostat's buffer)."""
        p = self._momenta(state)
        self._compute.kinetic(p, self._masses, self._idx_m, self.n_molecules, self._ke2, self._err, self._ws)
        return self._ke2.view(self.n_replicas, self.n_molecules)

    def state_dict(self):
        return {}

    def load_state_dict(self, sd):
        pass


class BerendsenThermostat(_ClassicalThermostat):
    """``BerendsenThermostat`` of the reference (thermostats.py:149-189): ``p <- p sqrt(1 + dt / tau (T0 / T - 1))`` per replica and
    molecule.  Deviation: a molecule without atoms or without kinetic energy keeps its momenta (the reference yields NaN there)."""

    def __init__(self, temperature_bath: float, time_constant: float, compute_fn=None, fs: float = FS_MD, kb: float = KB_MD):
        super().__init__(temperature_bath, time_constant, compute_fn, fs, kb)

    def apply(self, state, step: int = 0, which: int = 0, step_dev=None):
        p = self._momenta(state)
        c = self._compute
        c.kinetic(p, self._masses, self._idx_m, self.n_molecules, self._ke2, self._err, self._ws)
        c.berendsen_scale(self._ke2, self._n_atoms_mol, self.n_replicas, self.time_step / self.time_constant, self.temperature_bath, self.kb, self._scale)
        c.scale_molecules(p, self._scale, self._idx_m, self.n_molecules, self._err)
        return p


def langevin_coefficients(time_step: float, time_constant: float):
    """(c1, c2) of thermostats.py:226-237, float64: gamma = 1 / time_constant, c1 = exp(-dt/2 gamma), c2 = sqrt(1 - c1^2)."""
    c1 = torch.exp(-0.5 * time_step * (torch.ones(1, dtype=torch.float64) / time_constant))
    return c1, torch.sqrt(1.0 - c1 ** 2)


class LangevinThermostat(_ClassicalThermostat):
    """``LangevinThermostat`` of the reference (thermostats.py:192-261): ``p <- c1 p + sqrt(m kB T) c2 xi``.  No kernel of its own:
    this is ``spk_md_pile_f32`` at ONE bead with M = ([[c1]], [[c2]]) and noise_scale = sqrt(kB T) -- the centroid mode of PILE-L
    (whose friction 1 / time_constant does not depend on the ring-polymer frequency) is this thermostat.  Noise: that kernel's
    Philox stream keyed by (seed, step, which); ``step_dev`` for graph replays.  ``compute_fn`` has the signature of ``_pile_hip``."""

    def __init__(self, temperature_bath: float, time_constant: float, seed: int = 0, compute_fn=None, fs: float = FS_MD, kb: float = KB_MD):
        super().__init__(temperature_bath, time_constant, compute_fn, fs, kb)
        self.seed = int(seed)
        self.M = None

    @staticmethod
    def _default_compute():
        return _pile_hip

    def _init_thermostat(self):
        self.c1, self.c2 = langevin_coefficients(self.time_step, self.time_constant)
        self.M = torch.stack([self.c1.reshape(1, 1), self.c2.reshape(1, 1)]).float().contiguous()
        self.noise_scale = math.sqrt(self.kb * self.temperature_bath)

    def _prepare(self, state):
        p = state.momenta
        key = (p.device, p.dtype, tuple(p.shape))
        if self._ready == key:
            return
        if self.M is None:
            raise RuntimeError("LangevinThermostat.init(simulation_or_integrator) has not been called")
        n_rep, N = int(p.shape[0]), int(p.shape[1])
        self._M_dev = self.M.to(p.device, p.dtype)
        self._m_rep = state.masses.reshape(-1).to(p.device, p.dtype).repeat(n_rep).contiguous()
        if self._m_rep.numel() != n_rep * N:
            raise ValueError("masses: expected %d entries, got %d" % (N, self._m_rep.numel() // max(n_rep, 1)))
        self._out = torch.empty(1, n_rep * N, 3, dtype=p.dtype, device=p.device)
        self._ready = key

    def apply(self, state, step: int = 0, which: int = 0, step_dev=None):
        p = self._momenta(state)
        # replicas of a classical system are independent: one bead of n_replicas x n_atoms atoms, every component its own counter
        self._compute(p.view(1, -1, 3), self._m_rep, self._M_dev, self.noise_scale, self.seed, step, step_dev, which, 0, 1, self._out)
        with torch.no_grad():
            p.copy_(self._out.view(p.shape))
        return p


class NHCThermostat(_ClassicalThermostat):
    """``NHCThermostat`` of the reference (thermostats.py:264-511): a Nose-Hoover chain per (replica, molecule), or with ``massive``
    per momentum component, propagated by ``multi_step`` x ``integration_order`` Yoshida-Suzuki sub-steps.  The chain state lives in
    device tensors owned by this object; ``state_dict`` / ``load_state_dict`` expose it under the reference's buffer names and
    shapes (``velocities``, ``forces``, ``masses``: [n_replicas, n_molecules, 1, chain_length], massive [n_replicas, n_atoms, 3,
    chain_length]) so that a run can be continued.  ``integration_order`` 1 (one unsplit sub-step) is accepted on top of the
    reference's 3, 5, 7."""

    def __init__(self, temperature_bath: float, time_constant: float, chain_length: int = 3, massive: bool = False, multi_step: int = 2,
                 integration_order: int = 3, compute_fn=None, fs: float = FS_MD, kb: float = KB_MD):
        super().__init__(temperature_bath, time_constant, compute_fn, fs, kb)
        if int(chain_length) < 1:
            raise ValueError("chain_length must be at least 1")
        self.chain_length, self.massive = int(chain_length), bool(massive)
        self.multi_step, self.integration_order = int(multi_step), int(integration_order)
        nhc_sub_steps(1.0, self.multi_step, self.integration_order)          # validates both
        self.frequency = 1.0 / self.time_constant
        self.kb_temperature = self.temperature_bath * self.kb
        self.link_mass = self.kb_temperature / self.frequency ** 2
        self.sub_steps = None
        self._pending = None

    def _init_thermostat(self):
        self.sub_steps = nhc_sub_steps(self.time_step, self.multi_step, self.integration_order)

    def _prepare_thermostat(self, p):
        L = self.chain_length
        n = 3 * self.n_replicas * self.n_atoms if self.massive else self.n_replicas * self.n_molecules
        shape = (L, n) if self.massive else (n, L)          # massive: link-major, what the kernel reads coalesced
        self._vel = torch.zeros(shape, dtype=p.dtype, device=p.device)
        self._frc = torch.zeros(shape, dtype=p.dtype, device=p.device)
        if self._pending is not None:
            sd, self._pending = self._pending, None
            self.load_state_dict(sd)

    def _public(self, t):
        L = self.chain_length
        if self.massive:
            return t.t().reshape(self.n_replicas, self.n_atoms, 3, L)
        return t.reshape(self.n_replicas, self.n_molecules, 1, L)

    @property
    def degrees_of_freedom(self) -> torch.Tensor:
        if self.massive:
            return torch.ones(self.n_replicas, self.n_atoms, 3, dtype=torch.float64)
        return (3 * self._n_atoms_mol[None, :, None]).double().cpu()

    @property
    def masses(self) -> torch.Tensor:
        """Thermostat masses (thermostats.py:375-396): dof kT / omega^2 for the innermost link, kT / omega^2 for the rest (float64)."""
        dof = self.degrees_of_freedom
        m = torch.full(tuple(dof.shape) + (self.chain_length,), self.link_mass, dtype=torch.float64)
        m[..., 0] = dof * self.link_mass
        return m.expand(self.n_replicas, *m.shape[1:]).contiguous()

    def state_dict(self):
        if self._ready is None:
            raise RuntimeError("NHCThermostat: no chain state before the first application")
        return {"velocities": self._public(self._vel).clone(), "forces": self._public(self._frc).clone(), "masses": self.masses}

    def load_state_dict(self, sd):
        """Chain velocities and forces of an earlier run, copied INTO the owned buffers (a captured graph keeps pointing at them);
        before the first application they are kept and loaded when the buffers exist.  ``masses`` must be those of this thermostat."""
        if self._ready is None and getattr(self, "_vel", None) is None:
            self._pending = dict(sd)
            return
        want = tuple(self._public(self._vel).shape)
        for name, buf in (("velocities", self._vel), ("forces", self._frc)):
            t = sd[name]
            if tuple(t.shape) != want:
                raise ValueError("%s: expected shape %s, got %s" % (name, want, tuple(t.shape)))
            t = t.to(buf.device, buf.dtype)
            with torch.no_grad():
                buf.copy_(t.reshape(-1, self.chain_length).t() if self.massive else t.reshape(-1, self.chain_length))
        if "masses" in sd and not torch.allclose(sd["masses"].double().cpu(), self.masses, rtol=1e-5, atol=0.0):
            raise ValueError("masses of the loaded chain state are not those of this thermostat (temperature / time constant differ)")

    def apply(self, state, step: int = 0, which: int = 0, step_dev=None):
        p = self._momenta(state)
        c = self._compute
        args = (self.chain_length, self.multi_step, self.integration_order, self.sub_steps, self.kb_temperature, self.link_mass, self._vel, self._frc)
        if self.massive:
            c.nhc_massive(p, self._masses, *args)
        else:
            c.kinetic(p, self._masses, self._idx_m, self.n_molecules, self._ke2, self._err, self._ws)
            c.nhc_global(self._ke2, self._n_atoms_mol, self.n_replicas, *args, self._scale)
            c.scale_molecules(p, self._scale, self._idx_m, self.n_molecules, self._err)
        return p

    @property
    def scaling_factor(self) -> torch.Tensor:
        """Factor of the last global application, [n_replicas, n_molecules]."""
        return self._scale.view(self.n_replicas, self.n_molecules)


# ------------------------------------------------------------------------------------------------ ring-polymer thermostats beyond PILE-L
def rp_nhc_frequencies(n_beads: int, omega: float, time_constant: float) -> torch.Tensor:
    """Frequencies [B] (float64) behind the thermostat masses of ``NHCRingPolymerThermostat._init_masses``
    (md/simulation_hooks/thermostats_rpmd.py:417-455): the ring-polymer ``omega_normal`` (float32 sine, as the integrator forms it)
    with the centroid entry replaced by 0.5 / time_constant.  A private copy: the integrator's own frequencies are not touched (the
    reference overwrites ``integrator.omega_normal[0]`` in place, a side effect that is not reproduced)."""
    on = (2.0 * omega * torch.sin(torch.arange(n_beads).float() * math.pi / n_beads)).double()
    on[0] = 0.5 / time_constant
    return on


class _RingPolymerThermostatHip(_ThermostatHip):
    """Device side of the ring-polymer thermostats (csrc/spk_md_rp_thermo.hip) on top of the classical entries."""

    @staticmethod
    def centroid(p_all, p_c, xi_c, seed, step, step_dev, which):
        with torch.cuda.device(p_all.device):
            check(lib().spk_md_rp_centroid_f32(fptr(p_all), int(p_all.shape[0]), int(p_all.shape[1]), fptr(p_c), fptr(xi_c), int(seed), int(step),
                                               _lib.iptr(step_dev) if step_dev is not None else None, int(which), stream()))

    @classmethod
    def rp_nhc(cls, p_all, masses, C, link_masses, bead0, n_local, chain_length, multi_step, order, sub_steps, kT, vel, frc, scale_c, idx_m, n_mol, err, out):
        with torch.cuda.device(p_all.device):
            check(lib().spk_md_rp_nhc_f32(fptr(p_all), fptr(masses), fptr(C), fptr(link_masses), int(p_all.shape[0]), int(p_all.shape[1]), int(bead0),
                                          int(n_local), int(chain_length), int(multi_step), int(order), cls._steps(sub_steps), float(kT), fptr(vel), fptr(frc),
                                          fptr(scale_c), _lib.iptr(idx_m) if idx_m is not None else None, int(n_mol), _lib.iptr(err, torch.int32),
                                          fptr(out), stream()))

    @staticmethod
    def pile_alpha(ke2, noise2, xi_c, n_atoms_mol, first_atom, n_atoms, c1, one_minus_c1_kT, alpha, err):
        with torch.cuda.device(ke2.device):
            check(lib().spk_md_pile_alpha_f32(fptr(ke2), fptr(noise2), fptr(xi_c), _lib.iptr(n_atoms_mol), _lib.iptr(first_atom), int(n_atoms_mol.shape[0]),
                                              int(n_atoms), float(c1), float(one_minus_c1_kT), fptr(alpha), _lib.iptr(err, torch.int32), stream()))

    @staticmethod
    def pile_global(p_all, masses, M, noise_scale, seed, step, step_dev, which, bead0, n_local, p_c, alpha, idx_m, n_mol, err, out):
        with torch.cuda.device(p_all.device):
            check(lib().spk_md_pile_global_f32(fptr(p_all), fptr(masses), fptr(M), float(noise_scale), int(seed), int(step),
                                               _lib.iptr(step_dev) if step_dev is not None else None, int(which), int(p_all.shape[0]), int(p_all.shape[1]),
                                               int(bead0), int(n_local), fptr(p_c), fptr(alpha), _lib.iptr(idx_m), int(n_mol), _lib.iptr(err, torch.int32),
                                               fptr(out), stream()))


class _MoleculeLayoutRP:
    """The molecule layout of ONE bead and the centroid workspaces the global ring-polymer thermostats share (a mix-in without
    constructor arguments; the user sets ``n_beads`` and ``_compute``).

    Lifetime.  ``_set_layout`` (from ``init``) records the layout; with ``idx_m`` given, ``n_atoms`` / ``n_molecules`` are known from
    then on, without it (one molecule of all atoms) from the first ``prepare`` / application.  ``_prepare_layout`` allocates the device
    buffers once per (device, momenta shape) -- a thermostat made without ``idx_m`` follows a new atom count, one made with it
    refuses it.  The atom masses are copied INTO the owned buffer whenever another tensor, or the same tensor after an in-place
    write, is handed in: a captured graph keeps the buffer's address, and nobody is served the masses of an earlier call."""

    _layout_src = None            # (idx_m, n_atoms) as given to init, None: one molecule of all atoms
    _layout_ready = _masses_src = None
    _idx_m = _n_atoms_mol = None
    n_atoms = n_molecules = None

    def _set_layout(self, idx_m, n_atoms):
        if idx_m is not None:
            idx_m, n_atoms = idx_m.long().contiguous(), n_atoms.long().contiguous()
            if idx_m.numel() > 1 and bool((idx_m[1:] < idx_m[:-1]).any()):
                raise ValueError("idx_m must ascend (atoms of a molecule contiguous)")
            if idx_m.numel() and (int(idx_m.min()) < 0 or int(idx_m.max()) >= int(n_atoms.shape[0])):
                raise ValueError("idx_m outside [0, n_molecules)")
            self._layout_src = (idx_m, n_atoms)
            self.n_atoms, self.n_molecules = int(idx_m.shape[0]), int(n_atoms.shape[0])
        else:
            self._layout_src, self.n_atoms, self.n_molecules = None, None, None
        self._idx_m, self._n_atoms_mol = idx_m, n_atoms
        self._layout_ready = self._masses_src = None

    def _need_layout(self, what):
        if self.n_atoms is None:
            raise RuntimeError("%s.%s: the number of atoms is not known yet -- pass idx_m / n_atoms to init(), or call prepare(momenta, masses) "
                               "or apply the thermostat once" % (type(self).__name__, what))

    def _prepare_layout(self, p_all, masses) -> bool:
        """Buffers on the device of the momenta, allocated once per (device, shape); True when they are new."""
        key = (p_all.device, tuple(p_all.shape))
        new = self._layout_ready != key
        if new:
            if p_all.dim() != 3 or p_all.shape[2] != 3 or int(p_all.shape[0]) != self.n_beads:
                raise ValueError("momenta must be [n_beads = %d, n_atoms, 3]" % self.n_beads)
            N, dev = int(p_all.shape[1]), p_all.device
            idx_m, n_mol = self._layout_src or (torch.zeros(N, dtype=torch.long), torch.tensor([N], dtype=torch.long))
            if int(idx_m.shape[0]) != N:
                raise ValueError("idx_m has %d entries for %d atoms" % (int(idx_m.shape[0]), N))
            self._idx_m, self._n_atoms_mol = idx_m.to(dev), n_mol.to(dev)
            self._first_atom = (torch.cumsum(self._n_atoms_mol, 0) - self._n_atoms_mol).contiguous()
            self.n_atoms, self.n_molecules = N, int(self._n_atoms_mol.shape[0])
            self._masses = torch.empty(N, dtype=torch.float32, device=dev)
            self._masses_src = None
            self._ones = torch.ones(N, dtype=torch.float32, device=dev)
            self._p_c = torch.zeros(1, N, 3, dtype=torch.float32, device=dev)
            self._xi_c = torch.zeros(1, N, 3, dtype=torch.float32, device=dev)
            self._ke2 = torch.zeros(self.n_molecules, dtype=torch.float32, device=dev)
            self._s2 = torch.zeros(self.n_molecules, dtype=torch.float32, device=dev)
            self._scale = torch.ones(self.n_molecules, dtype=torch.float32, device=dev)
            self._err = torch.zeros(1, dtype=torch.int32, device=dev)
            self._ws = self._compute.workspace(1, N, self.n_molecules, dev)
            self._layout_ready = key
        # the source tensor is held, so "the same object at the same version" cannot be another tensor in recycled memory
        if self._masses_src is None or self._masses_src[0] is not masses or self._masses_src[1] != masses._version:
            with torch.no_grad():
                self._masses.copy_(_flat_masses(masses, self.n_atoms))
            self._masses_src = (masses, masses._version)
        return new

    def centroid_kinetic2(self, p_all, masses) -> torch.Tensor:
        """sum over the atoms of a molecule of |p_c|^2 / m for the centroid normal-mode momentum p_c = sum_b p_b / sqrt(B), [n_molecules]
        (a view of the thermostat's buffer)."""
        p_all = p_all.contiguous()
        self._prepare_layout(p_all, masses)
        self._compute.centroid(p_all, self._p_c, None, 0, 0, None, 0)
        self._compute.kinetic(self._p_c, self._masses, self._idx_m, self.n_molecules, self._ke2, self._err, self._ws)
        return self._ke2


class _RingPolymerThermostat(_MoleculeLayoutRP):
    """What the ring-polymer thermostats of csrc/spk_md_rp_thermo.hip share: bath temperature, time constant in fs, the bead range of
    a bead-parallel group and ``apply`` = ONE all-gather of the momenta + ``apply_beads`` (as ``PILELocalThermostat``)."""

    ring_polymer = True

    def __init__(self, temperature_bath: float, time_constant: float, group=None, compute_fn=None, fs: float = FS_MD, kb: float = KB_MD):
        self.temperature_bath, self.time_constant = float(temperature_bath), float(time_constant) * float(fs)
        self.kb, self.group = float(kb), group
        self._compute = compute_fn or _RingPolymerThermostatHip
        self.n_beads = None

    def init(self, integrator: RingPolymer, idx_m: Optional[torch.Tensor] = None, n_atoms: Optional[torch.Tensor] = None):
        self.n_beads, self.time_step, self.omega = integrator.n_beads, float(integrator.time_step), float(integrator.omega)
        self.kb_temperature = self.kb * self.n_beads * self.temperature_bath          # kT of the ring polymer: n_beads kB T
        self._range = integrator._bead_range if self.group is None else RingPolymer(integrator.time_step, self.n_beads, 1.0, omega=1.0,
                                                                                    group=self.group)._bead_range
        self._set_layout(idx_m, n_atoms)
        self._init_thermostat()
        return self

    def _init_thermostat(self):
        pass

    def prepare(self, p_all, masses):
        self._prepare_layout(p_all, masses)

    def apply(self, state, step: int = 0, which: int = 0, step_dev=None, out=None):
        return _apply_to_state(self, state, step, which, step_dev, out)

    def state_dict(self):
        return {}

    def load_state_dict(self, sd):
        pass


class NHCRingPolymerThermostat(_RingPolymerThermostat):
    """``NHCRingPolymerThermostat`` of the reference (md/simulation_hooks/thermostats_rpmd.py:373-501): the massive Nose-Hoover chain
    on the NORMAL-MODE momenta, kT = n_beads kB T, every link of mode k with the mass kT / omega_k^2 (``rp_nhc_frequencies``).
    ``local=False``: the centroid of every molecule is ONE chain on the molecule's whole centroid kinetic energy with 3 n_atoms
    degrees of freedom (``spk_md_nhc_global_f32``).  One launch (``spk_md_rp_nhc_f32``) transforms, propagates every chain, scales and
    transforms back; the chain state of ALL modes lives on every rank of a bead-parallel run and is advanced identically there.

    ``state_dict`` / ``load_state_dict``: ``velocities`` / ``forces`` / ``masses`` in the reference's shape [n_beads, n_atoms, 3,
    chain_length]; with ``local=False`` the centroid rows are the molecule chains broadcast over their atoms (loading takes them
    from the first atom of every molecule).  The reference's in-place edit of the integrator's ``omega_normal[0]`` is not
    reproduced: the ``RingPolymer`` propagator stays as it is.  ``integration_order`` 1 is accepted on top of 3, 5, 7."""

    def __init__(self, temperature_bath: float, time_constant: float, local: bool = True, chain_length: int = 3, multi_step: int = 2,
                 integration_order: int = 3, group=None, compute_fn=None, fs: float = FS_MD, kb: float = KB_MD):
        super().__init__(temperature_bath, time_constant, group, compute_fn, fs, kb)
        if int(chain_length) < 1:
            raise ValueError("chain_length must be at least 1")
        self.local, self.chain_length = bool(local), int(chain_length)
        self.multi_step, self.integration_order = int(multi_step), int(integration_order)
        nhc_sub_steps(1.0, self.multi_step, self.integration_order)          # validates both
        self.frequency = 1.0 / self.time_constant
        self.sub_steps = None
        self._vel = self._frc = None
        self._pending = None

    def _init_thermostat(self):
        self.sub_steps = nhc_sub_steps(self.time_step, self.multi_step, self.integration_order)
        self.frequencies = rp_nhc_frequencies(self.n_beads, self.omega, self.time_constant)
        self.link_masses = self.kb_temperature / self.frequencies ** 2                  # [B] float64
        self.C = normal_mode_matrix(self.n_beads).float().contiguous()
        self._vel = self._frc = None

    def prepare(self, p_all, masses):
        if not self._prepare_layout(p_all, masses) and self._vel is not None:
            return
        if self.sub_steps is None:
            raise RuntimeError("NHCRingPolymerThermostat.init(integrator) has not been called")
        dev, L, B, N = p_all.device, self.chain_length, self.n_beads, self.n_atoms
        self._C_dev, self._lm_dev = self.C.to(dev), self.link_masses.float().to(dev)
        self._vel = torch.zeros(L, B, 3 * N, dtype=torch.float32, device=dev)         # link-major: what the kernel reads coalesced
        self._frc = torch.zeros(L, B, 3 * N, dtype=torch.float32, device=dev)
        self._cvel = torch.zeros(self.n_molecules, L, dtype=torch.float32, device=dev)   # local=False: the molecules' centroid chains
        self._cfrc = torch.zeros(self.n_molecules, L, dtype=torch.float32, device=dev)
        if self._pending is not None:
            sd, self._pending = self._pending, None
            self.load_state_dict(sd)

    @property
    def degrees_of_freedom(self) -> torch.Tensor:
        """[n_beads, n_atoms, 3] (float64): 1, and 3 n_atoms of the atom's molecule on the global centroid.  Needs the atom count:
        ``init`` with ``idx_m``, or the first ``prepare`` / application (RuntimeError before)."""
        self._need_layout("degrees_of_freedom")
        dof = torch.ones(self.n_beads, self.n_atoms, 3, dtype=torch.float64)
        if not self.local:
            dof[0] = (3 * self._n_atoms_mol[self._idx_m]).double().cpu()[:, None]
        return dof

    @property
    def masses(self) -> torch.Tensor:
        """Thermostat masses [n_beads, n_atoms, 3, chain_length] (float64): kT / omega_k^2, innermost link x degrees of freedom.
        Available when ``degrees_of_freedom`` is."""
        self._need_layout("masses")
        m = self.link_masses[:, None, None, None].expand(self.n_beads, self.n_atoms, 3, self.chain_length).clone()
        m[..., 0] *= self.degrees_of_freedom
        return m

    def _public(self, t, ct):
        L, B, N = self.chain_length, self.n_beads, self.n_atoms
        out = t.permute(1, 2, 0).reshape(B, N, 3, L).clone()
        if not self.local:
            out[0] = ct[self._idx_m][:, None, :].expand(N, 3, L)
        return out

    def state_dict(self):
        if self._vel is None:
            raise RuntimeError("NHCRingPolymerThermostat: no chain state before the buffers exist (prepare / first application)")
        return {"velocities": self._public(self._vel, self._cvel), "forces": self._public(self._frc, self._cfrc), "masses": self.masses}

    def load_state_dict(self, sd):
        """Chain state of an earlier run, copied INTO the owned buffers (a captured graph keeps pointing at them); before the
        buffers exist it is kept and loaded when they do."""
        if self._vel is None:
            self._pending = dict(sd)
            return
        L, B, N = self.chain_length, self.n_beads, self.n_atoms
        live = self._n_atoms_mol > 0
        for name, buf, cbuf in (("velocities", self._vel, self._cvel), ("forces", self._frc, self._cfrc)):
            t = sd[name]
            if tuple(t.shape) != (B, N, 3, L):
                raise ValueError("%s: expected shape %s, got %s" % (name, (B, N, 3, L), tuple(t.shape)))
            t = t.to(buf.device, buf.dtype)
            with torch.no_grad():
                if self.local:
                    buf.copy_(t.reshape(B, 3 * N, L).permute(2, 0, 1))
                else:
                    buf[:, 1:].copy_(t[1:].reshape(B - 1, 3 * N, L).permute(2, 0, 1))
                    cbuf[live] = t[0, self._first_atom[live], 0, :]
        if "masses" in sd and not torch.allclose(sd["masses"].double().cpu(), self.masses, rtol=1e-5, atol=0.0):
            raise ValueError("masses of the loaded chain state are not those of this thermostat (temperature / time constant differ)")

    def apply_beads(self, p_all, masses, bead0, n_local, step=0, step_dev=None, which=0, out=None):
        self.prepare(p_all, masses)
        c = self._compute
        if out is None:
            out = torch.empty(n_local, self.n_atoms, 3, dtype=torch.float32, device=p_all.device)
        chain = (self.chain_length, self.multi_step, self.integration_order, self.sub_steps, self.kb_temperature)
        scale = None
        if not self.local:
            c.centroid(p_all, self._p_c, None, 0, 0, None, 0)
            c.kinetic(self._p_c, self._masses, self._idx_m, self.n_molecules, self._ke2, self._err, self._ws)
            c.nhc_global(self._ke2, self._n_atoms_mol, 1, *chain, float(self.link_masses[0]), self._cvel, self._cfrc, self._scale)
            scale = self._scale
        c.rp_nhc(p_all, self._masses, self._C_dev, self._lm_dev, bead0, n_local, *chain, self._vel, self._frc, scale,
                 self._idx_m, self.n_molecules, self._err, out)
        return out

    @property
    def scaling_factor(self) -> torch.Tensor:
        """Centroid factor of the last ``local=False`` application, [n_molecules]."""
        return self._scale


class PILEGlobalThermostat(_MoleculeLayoutRP, PILELocalThermostat):
    """``PILEGlobalThermostat`` of the reference (md/simulation_hooks/thermostats_rpmd.py:122-208): PILE-L on the modes k >= 1 (same
    coefficients, same Philox counters as ``PILELocalThermostat`` with the same seed) and, on the centroid of every molecule, the
    stochastic velocity rescaling of Bussi, Donadio and Parrinello: p_c <- alpha p_c with

        alpha^2 = c + S g + 2 R1 sqrt(c g),  alpha = sqrt(alpha^2) sign(R1 + sqrt(c / g)),  g = (1 - c) n_beads kB T / K

    K = the molecule's centroid kinetic sum, S = the sum of its squared centroid noise, c = c1[0].

    Two deviations from the reference.  (1) R1 of a molecule is the centroid noise of the x component of ITS first atom.  The
    reference takes element [0, 0, 0] of the batch's noise -- atom 0 of the whole batch -- for every molecule, which couples the
    molecules of a batch and gives all but the first an R1 that is not among its own S terms (not Bussi's distribution); for one
    molecule the two coincide.  (2) A molecule without atoms or with K = 0 (every run starts from zero momenta) gets alpha = 1: its
    centroid is left alone and no noise is added there; the reference divides by zero."""

    def __init__(self, temperature_bath: float, time_constant: float, seed: int = 0, group=None, compute_fn=None, fs: float = FS_MD,
                 kb: float = KB_MD):
        # the layout mix-in takes no arguments; PILE-L's constructor does everything, with the device entries of this class as ``compute_fn``
        super().__init__(temperature_bath, time_constant, True, 1.0, seed, group, compute_fn or _RingPolymerThermostatHip, fs, kb)

    def init(self, integrator: RingPolymer, idx_m: Optional[torch.Tensor] = None, n_atoms: Optional[torch.Tensor] = None):
        super().init(integrator)
        self.kb_temperature = self.kb * self.n_beads * self.temperature_bath
        self._set_layout(idx_m, n_atoms)
        self._M_dev = None
        return self

    def _matrices(self, integrator):
        """M of PILE-L with the centroid taken out (c1[0] = c2[0] = 0); c1[0] goes to the rescaling."""
        C = normal_mode_matrix(self.n_beads)
        c1, c2 = pile_coefficients(self.n_beads, integrator.omega, integrator.time_step, self.time_constant, True, 1.0)
        self.c1_centroid = float(c1[0])
        c1, c2 = c1.clone(), c2.clone()
        c1[0] = c2[0] = 0.0
        return torch.stack([C.t() @ torch.diag(c1) @ C, C.t() @ torch.diag(c2)]).float().contiguous()

    def prepare(self, p_all, masses):
        self._prepare_layout(p_all, masses)
        if self._M_dev is None or self._M_dev.device != p_all.device:
            self._M_dev = self.M.to(p_all.device)

    def apply_beads(self, p_all, masses, bead0, n_local, step=0, step_dev=None, which=0, out=None):
        self.prepare(p_all, masses)
        c = self._compute
        if out is None:
            out = torch.empty(n_local, self.n_atoms, 3, dtype=torch.float32, device=p_all.device)
        c.centroid(p_all, self._p_c, self._xi_c, self.seed, step, step_dev, which)
        c.kinetic(self._p_c, self._masses, self._idx_m, self.n_molecules, self._ke2, self._err, self._ws)
        c.kinetic(self._xi_c, self._ones, self._idx_m, self.n_molecules, self._s2, self._err, self._ws)
        c.pile_alpha(self._ke2, self._s2, self._xi_c, self._n_atoms_mol, self._first_atom, self.n_atoms, self.c1_centroid,
                     (1.0 - self.c1_centroid) * self.kb_temperature, self._scale, self._err)
        c.pile_global(p_all, self._masses, self._M_dev, self.noise_scale, self.seed, step, step_dev, which, bead0, n_local, self._p_c,
                      self._scale, self._idx_m, self.n_molecules, self._err, out)
        return out

    @property
    def alpha(self) -> torch.Tensor:
        """Centroid factor of the last application, [n_molecules]."""
        return self._scale


class TRPMDThermostat(PILELocalThermostat):
    """``TRPMDThermostat`` of the reference (md/simulation_hooks/thermostats_rpmd.py:211-234): PILE-L without a centroid thermostat
    and with the friction of the modes k >= 1 multiplied by ``damping_factor`` -- ``PILELocalThermostat(temperature_bath, 1.0,
    thermostat_centroid=False, damping_factor=damping_factor)``, bit for bit."""

    def __init__(self, temperature_bath: float, damping_factor: float, seed: int = 0, group=None, compute_fn=None, fs: float = FS_MD,
                 kb: float = KB_MD):
        super().__init__(temperature_bath, 1.0, False, damping_factor, seed, group, compute_fn, fs, kb)


class MDState:
    """Minimal stand-in for ``schnetpack.md.System`` (md/system.py): the tensors the integrators touch."""

    def __init__(self, positions, momenta, masses, forces=None):
        self.positions, self.momenta, self.masses = positions, momenta, masses
        self.forces = forces if forces is not None else torch.zeros_like(positions)


class NVESimulation:
    """The inner loop of ``md.Simulator.simulate`` (md/simulator.py:124-157) for plain NVE dynamics of ONE
    batch of systems on one GPU, everything resident on the device.  One MD step is ONE HIP-graph replay

        kick + drift + skin test (1 kernel)  ->  force call on the current list  ->  kick (1 kernel)

    and every ``check_every`` steps (adapted to the dynamics, at most ``max_check_every``) one two-word D2H read -- the only
    host synchronisation of the loop.  Because the skin flag is read up to ``check_every`` steps AFTER it came up, the rebuild
    threshold is ``shell / 2 - margin`` with ``margin`` at least twice (usually four times) ``check_every`` x the largest
    one-step displacement seen (tracked by the kick-drift kernel): when the flag is read, the forces of all steps since it
    came up were still computed with a valid list, and the list is rebuilt (and the graph re-captured) before the next
    step.  A displacement that exceeds the margin raises.

    Batches of small isolated molecules (no cell, at most 28 atoms each -- every pair of a molecule then fits the molecule-
    resident kernels) skip the skin machinery altogether (``complete_list="auto"``): the list holds EVERY intramolecular pair,
    which is a Verlet list with an infinite skin -- pairs beyond the cutoff contribute exactly zero (the kernels do not even give
    them a tile) -- so it never has to be rebuilt, the kick-drift kernel tests nothing, and the loop is back-to-back graph
    replays without a host synchronisation.

    ``inputs`` is the batch dict on the device with ``_positions`` [N,3], ``_atomic_numbers``, ``_idx_m``,
    ``_n_atoms`` and (periodic) ``_cell`` / ``_pbc``; positions, masses, time step and the model's energy
    must share one unit system (forces = -dE/dpositions)."""

    def __init__(self, model, inputs, masses, time_step, cutoff, cutoff_shell=1.0, use_graph=True, max_check_every=4,
                 complete_list="auto"):
        from . import properties
        from .neighborlist import NeighborListMD
        self.P = properties
        self._complete = self._wants_complete_list(inputs, complete_list)
        self.max_check_every = max(int(max_check_every), 1)
        self.check_every = 1            # raised once the displacement scale is known
        self.model = model.eval()
        self.inputs = dict(inputs)
        R = inputs[properties.R].detach().float().contiguous().clone()
        self._time_step = time_step
        self._setup_state(R, masses)
        self.nl = NeighborListMD(cutoff, cutoff_shell, filter_buffer=False)
        self.use_graph = use_graph
        self.flag = torch.zeros(2, dtype=torch.int32, device=R.device)
        self.n_molecules = int(inputs[properties.n_atoms].shape[0])
        self.margin = 0.25 * cutoff_shell      # adapted to 4 x the largest one-step displacement once steps have run
        self.energy = None
        self.graph = None
        self.n_captures = 0
        self.t_rebuild = 0.0          # wall time spent in list rebuilds + graph re-captures (synchronised)
        self._lists = None
        self._rebuild()

    def _setup_state(self, R, masses):
        self.state = MDState(R.unsqueeze(0), torch.zeros_like(R).unsqueeze(0), masses.float().reshape(1, -1, 1))
        self.integrator = VelocityVerlet(self._time_step)

    # -- complete intramolecular lists ---------------------------------------------------------
    MAX_COMPLETE_ATOMS = 28        # 28 * 27 / 2 = 378 pairs <= the 384 pairs a group of the molecule-resident kernels holds

    def _wants_complete_list(self, inputs, mode) -> bool:
        P = self.P
        if mode is False or mode is None:
            return False
        pbc = inputs.get(P.pbc)
        periodic = inputs.get(P.cell) is not None and pbc is not None and bool(pbc.any())
        small = int(inputs[P.n_atoms].max()) <= self.MAX_COMPLETE_ATOMS
        if mode is True and (periodic or not small):
            raise ValueError("complete_list=True needs isolated molecules of at most %d atoms" % self.MAX_COMPLETE_ATOMS)
        return (not periodic) and small

    @staticmethod
    def complete_pair_list(idx_m: torch.Tensor, n_atoms: torch.Tensor):
        """Every ordered pair (i, j), i != j, of atoms of the same molecule; idx_i ascending, idx_j ascending within a row --
        the order of the reference's neighbour lists (atoms of a molecule are contiguous)."""
        dev = idx_m.device
        N = int(idx_m.shape[0])
        start = torch.cumsum(n_atoms, 0) - n_atoms                   # first atom of every molecule
        counts = n_atoms[idx_m] - 1                                  # partners per atom
        idx_i = torch.repeat_interleave(torch.arange(N, device=dev), counts)
        seg = torch.cumsum(counts, 0) - counts
        k = torch.arange(int(idx_i.shape[0]), device=dev) - seg[idx_i]
        first = start[idx_m[idx_i]]
        idx_j = first + k + (k >= (idx_i - first)).long()
        return idx_i, idx_j

    # -- pieces of one step ------------------------------------------------------------------
    def _flatR(self):
        return self.state.positions.view(-1, 3)

    def _call_inputs(self):
        call = dict(self.inputs)
        call.update(self._lists)
        call[self.P.R] = self._flatR()                    # the state tensor itself: no copy per step
        call["_n_molecules"] = self.n_molecules
        return call

    def _force_eval(self):
        out = self.model(self._call_inputs())
        with torch.no_grad():
            self._f.copy_(out["forces"].detach())
            self._e.copy_(out["energy"].detach())

    def _prepare_plan(self):
        """Edge plan (CSR, reverse map, skin-filter decision) of the current list without a full force call: warms the
        plan cache of the operator library outside any graph capture (one host sync per new list)."""
        P = self.P
        R = self._flatR()
        ii, jj = self._lists[P.idx_i], self._lists[P.idx_j]
        with torch.no_grad():
            r = torch.ops.spk_hip.pairwise(R.detach(), ii, jj, self._lists.get(P.offsets))
            rep = getattr(self.model, "representation", None)
            cutoff = 0.0
            if rep is not None and hasattr(rep, "cutoff_fn") and hasattr(rep.cutoff_fn, "cutoff_value"):
                cutoff = float(rep.cutoff_fn.cutoff_value())
            torch.ops.spk_hip.edge_plan(ii, jj, int(R.shape[0]), r, cutoff)
            if getattr(self.model, "_potential_forces", False):      # the energy-store decision of the fused potential: one D2H, now
                torch.ops.spk_hip.potential_plan(ii, jj, int(R.shape[0]), self.inputs[P.idx_m], self.n_molecules)

    def _step_body(self):
        if self._complete:
            self.integrator.first_half_and_main_step(self.state, True)
        else:
            thr = max(0.5 * self.nl.cutoff_shell - self.margin, 0.0)
            self.integrator.first_half_and_main_step(self.state, True, self.nl.previous_positions, thr, self.flag)
        self._force_eval()
        self.integrator.half_step(self.state)

    def _rebuild(self, new_list=True):
        import time
        t0 = time.perf_counter()
        P = self.P
        self.graph = None
        if new_list and self._complete:
            ii, jj = self.complete_pair_list(self.inputs[P.idx_m], self.inputs[P.n_atoms])
            self._lists = {P.idx_i: ii, P.idx_j: jj, P.offsets: torch.zeros(ii.shape[0], 3, device=ii.device)}
            self.nl.n_builds += 1
        elif new_list:
            self.inputs[P.R] = self._flatR()
            self.nl._list = None
            self._lists = self.nl.get_neighbors(self.inputs)
            self.flag.zero_()
        if not new_list:
            pass
        elif self.energy is None:
            out = self.model(self._call_inputs())              # first call: builds the plan, sizes the outputs
            self._f = self._force_buffer(out["forces"].detach())
            self._e = out["energy"].detach().clone()
            self.energy = self._e
        else:
            self._prepare_plan()                               # plan of the new list (host syncs) outside any capture
        if self.use_graph:
            # capture records without executing: positions / momenta are untouched
            if self.n_captures == 0:
                torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._step_body()
            self.graph = g
            self.n_captures += 1
        torch.cuda.synchronize(self.flag.device)
        self.t_rebuild += time.perf_counter() - t0

    def _force_buffer(self, f):
        """Static force buffer the captured force call writes into ([N, 3]; the state's ``forces`` is a view of it)."""
        buf = f.clone()
        self.state.forces = buf.view(self.state.positions.shape)
        return buf

    def _one_step(self):
        if self.graph is not None:
            self.graph.replay()
        else:
            self._step_body()

    def step(self, n_steps=1):
        import time
        if self._complete:                     # nothing to watch: back-to-back replays, no host synchronisation
            for _ in range(n_steps):
                self._one_step()
            return
        done = 0
        while done < n_steps:
            k = min(self.check_every, n_steps - done)
            t0 = time.perf_counter()
            for _ in range(k):
                self._one_step()
            done += k
            moved, step_bits = self.flag.tolist()              # the one host sync of the chunk
            t_step = (time.perf_counter() - t0) / k
            step_disp = math.sqrt(struct.unpack("f", struct.pack("i", step_bits))[0])
            if k * step_disp > self.margin:
                raise RuntimeError("MD: an atom moved by up to %.3g per step over %d unchecked steps, more than the skin margin %.3g: "
                                   "reduce the time step or increase cutoff_shell" % (step_disp, k, self.margin))
            shell = self.nl.cutoff_shell
            # steps between two looks at the flag: the host round trip (tens of microseconds) matters for sub-millisecond steps
            # only, and every unchecked step costs margin (= earlier rebuilds): a few for small systems, one for large ones,
            # never more than keep 2 k x the step displacement below a twentieth of the skin
            kmax = int(0.05 * shell / (2.0 * step_disp)) if step_disp > 0.0 else self.max_check_every
            self.check_every = max(1, min(self.max_check_every, kmax, int(1.2e-3 / max(t_step, 1e-6))))
            # hysteresis: margin >= 2 x check_every x the largest one-step displacement at all times (and a floor that grows with
            # check_every: speeds may still be ramping up), re-tuned (= one re-capture, the threshold is baked into the captured
            # kernel) only when the displacement scale changed by 2x
            need = min(max(2.0 * self.check_every * step_disp, 0.0125 * self.check_every * shell), 0.45 * shell)
            retune = need > self.margin or 8.0 * need < self.margin
            if retune:
                self.margin = min(2.0 * need, 0.45 * shell)
            if moved:
                self._rebuild(True)
            elif retune:
                self._rebuild(False)

    def kinetic_energy(self):
        p, m = self.state.momenta, self.state.masses.reshape(1, -1, 1)
        return 0.5 * (p * p / m).sum()

    def total_energy(self):
        return float(self.energy.sum() + self.kinetic_energy())


class NVTSimulation(NVESimulation):
    """Classical dynamics at a set temperature: ``NVESimulation`` with a thermostat hook at the begin and the end of every step, in
    the order of the reference's ``Simulator.simulate`` (md/simulator.py:124-150):

        thermostat  ->  kick + drift + skin test (1 kernel)  ->  force call  ->  kick  ->  thermostat  ->  step counter += 1

    all of it ONE HIP-graph replay with ``use_graph=True``.  The skin / complete-list machinery is the parent's, untouched; a list
    rebuild re-captures the step around the same chain-state and step-counter tensors.  ``thermostat``: ``BerendsenThermostat``,
    ``LangevinThermostat`` or ``NHCThermostat`` (None: plain NVE).  The step counter is a device word incremented inside the
    captured step (fresh Langevin noise per replay).  Ring-polymer thermostats, GLE and barostats are refused: ``RPMDSimulation``
    keeps PILE-L, the other two are not built."""

    def __init__(self, model, inputs, masses, time_step, cutoff, thermostat=None, cutoff_shell=1.0, use_graph=True, max_check_every=4,
                 complete_list="auto", barostat=None):
        if barostat is not None or getattr(thermostat, "pressure_control", False):
            raise NotImplementedError("NVTSimulation: barostats (NPT) are not built; a strained cell changes the neighbour-list contract")
        if thermostat is not None:
            if getattr(thermostat, "ring_polymer", False):
                raise ValueError("NVTSimulation integrates classical states: %s is a ring-polymer thermostat (use RPMDSimulation)"
                                 % type(thermostat).__name__)
            if not isinstance(thermostat, _ClassicalThermostat):
                raise NotImplementedError("NVTSimulation: thermostat must be a BerendsenThermostat, LangevinThermostat or NHCThermostat "
                                          "(GLE is not built), got %s" % type(thermostat).__name__)
        self.thermostat = thermostat
        super().__init__(model, inputs, masses, time_step, cutoff, cutoff_shell, use_graph, max_check_every, complete_list)

    def _setup_state(self, R, masses):
        super()._setup_state(R, masses)
        self._stepc = torch.zeros(1, dtype=torch.int64, device=R.device)
        kb = self.thermostat.kb if self.thermostat is not None else KB_MD
        self._meter = _ClassicalThermostat(0.0, 1.0, kb=kb).init(self)
        self._meter._prepare(self.state)
        if self.thermostat is not None:          # buffers before the first capture
            self.thermostat.init(self)
            self.thermostat._prepare(self.state)

    def _step_body(self):
        th = self.thermostat
        if th is not None:
            th.apply(self.state, 0, 0, self._stepc)
        super()._step_body()
        if th is not None:
            th.apply(self.state, 0, 1, self._stepc)
        with torch.no_grad():
            self._stepc.add_(1)

    @property
    def step_count(self) -> int:
        return int(self._stepc.item())

    def kinetic_energy(self) -> torch.Tensor:
        """Kinetic energy per molecule, [n_molecules] (``spk_md_kinetic_f32``; ``System.kinetic_energy``, md/system.py:374-386)."""
        return 0.5 * self._meter.kinetic_energy2(self.state).reshape(-1)

    def temperature(self) -> torch.Tensor:
        """Instantaneous temperature per molecule, [n_molecules] (md/system.py:407-421); 0 for a molecule without atoms."""
        ke2 = self._meter.kinetic_energy2(self.state).reshape(-1)
        n = self._meter._n_atoms_mol.to(ke2.dtype)
        return torch.where(n > 0, ke2 / (3.0 * n.clamp_min(1.0) * self._meter.kb), torch.zeros_like(ke2))

    def total_energy(self):
        return float(self.energy.sum() + self.kinetic_energy().sum())


def fold_replicas(inputs, n_beads: int):
    """``n_beads`` replicas of a batch folded into the batch dimension, replica-major, as the reference's
    ``MDCalculator._get_system_molecules`` does (md/calculators/base_calculator.py:154-194): atom types, atom counts, cells and
    pbc repeated, ``idx_m`` of replica r shifted by ``r * n_molecules``.  Every replica starts at the positions given."""
    from . import properties as P
    B = int(n_beads)
    n_mol = int(inputs[P.n_atoms].shape[0])
    rep = dict(inputs)
    rep[P.R] = inputs[P.R].detach().float().repeat(B, 1)
    rep[P.Z] = inputs[P.Z].repeat(B)
    rep[P.idx_m] = (inputs[P.idx_m][None, :] + n_mol * torch.arange(B, device=inputs[P.idx_m].device)[:, None]).reshape(-1)
    rep[P.n_atoms] = inputs[P.n_atoms].repeat(B)
    if inputs.get(P.cell) is not None:
        rep[P.cell] = inputs[P.cell].reshape(-1, 3, 3).repeat(B, 1, 1)
    if inputs.get(P.pbc) is not None:
        rep[P.pbc] = inputs[P.pbc].reshape(-1, 3).repeat(B, 1).reshape(-1)
    return rep


class RPMDSimulation(NVESimulation):
    """Ring-polymer MD (md/integrators.py:113-229) of ``n_beads`` replicas of ONE batch of systems: the beads are folded
    into the batch dimension exactly as the reference does (md/calculators/base_calculator.py:166-183), so one force call
    and one device neighbour list serve all beads of a rank.  Single process -- one step is one graph replay:

        [thermostat]  ->  kick (p += dt/2 F)  ->  ring-polymer main step (k_md_ring_polymer: bead mixing + skin test)  ->
        force call of all beads  ->  kick  ->  [thermostat]

    ``thermostat``: ``PILELocalThermostat``, ``PILEGlobalThermostat``, ``TRPMDThermostat`` or ``NHCRingPolymerThermostat``; the
    simulation hands every one of them the momenta of all beads, the rank's bead range, the device step counter and its output
    buffer (``apply_beads``).  GLE and PIGLET are not built.  ``centroid_kinetic_energy()`` / ``centroid_temperature()`` per molecule
    work where this process holds the momenta of all beads (single process, ``exchange="forces"``); with ``exchange="state"`` over
    several ranks they raise NotImplementedError.

    The conserved quantity (no thermostat) is the ring-polymer Hamiltonian
    ``sum_b [p_b^2 / 2m + V(q_b)] + sum_b 1/2 m omega^2 |q_b - q_{b+1}|^2`` (``total_energy``).

    **Bead-parallel** (``group`` given; SURVEY.md section 8(e): one contiguous chunk of ``n_beads / world`` beads per rank,
    each rank with its own neighbour list and its own force-call graph; the normal-mode mixing
    md/utils/normal_model_transformation.py:70-98 is the only thing that couples beads).  Two exchange schemes:

    * ``exchange="state"`` -- every rank holds ONLY its beads.  One all-gather of the packed (positions, momenta) in the
      ring-polymer main step (``RingPolymer(group=...)``) and one all-gather of the momenta per application of the
      thermostat (``PILELocalThermostat(group=...)``): 1 + applications = 3 collectives per NVT step, 1 per NVE step --
      the reference's three exchange points (md/simulator.py:126-150), nothing more.
    * ``exchange="forces"`` -- every rank carries the integrator state of ALL beads (``n_beads x N x 3`` floats: 3 MB at
      configs[4]) and repeats the element-wise integrator / thermostat arithmetic, which is bit-identical on every rank
      (deterministic kernels, counter-based noise); only the FORCE CALL is sharded, so the one exchange of a step is the
      all-gather of the forces: 1 collective per step with or without the thermostat.

    Collectives are counted in ``n_collectives``.  The force call (+ the kernels next to it) of a rank is a HIP graph; the
    collectives run between the graph segments (RCCL on its own stream; ``gloo`` staged through the host so that two ranks
    can share one device in a test)."""

    def __init__(self, model, inputs, masses, time_step, n_beads, cutoff, temperature=300.0, omega=None,
                 cutoff_shell=1.0, use_graph=True, thermostat=None, complete_list="auto",
                 group=None, exchange: str = "state"):
        from . import properties as P
        if exchange not in ("state", "forces"):
            raise ValueError("exchange must be 'state' or 'forces'")
        self.thermostat = thermostat
        self.n_beads = int(n_beads)
        self.group, self.exchange = group, exchange
        self.n_collectives = 0
        self._rp = RingPolymer(time_step, self.n_beads, temperature, omega=omega, group=group)
        self._lo, hi, self._world = self._rp._bead_range()
        # the distributed code path: several ranks -- or ONE rank with a group when SPK_MD_FORCE_COLLECTIVES=1 (the RCCL smoke test of a one-GPU
        # box: every all-gather then executes, as an identity, on the real back-end)
        self._dist = self._world > 1 or (group is not None and os.environ.get("SPK_MD_FORCE_COLLECTIVES") == "1")
        self.n_local = B = hi - self._lo                      # beads in THIS rank's batch
        N = int(inputs[P.R].shape[0])
        rep = fold_replicas(inputs, B)
        self._n1 = N
        self._idx_m1, self._n_atoms1 = inputs[P.idx_m].long().contiguous(), inputs[P.n_atoms].long().contiguous()   # layout of ONE bead
        super().__init__(model, rep, masses, time_step, cutoff, cutoff_shell, use_graph, complete_list=complete_list)

    # -- state ---------------------------------------------------------------------------------
    @property
    def _replicated(self) -> bool:
        return self._dist and self.exchange == "forces"

    def _setup_state(self, R, masses):
        Bl, N, dev = self.n_local, self._n1, R.device
        m = masses.float().reshape(1, -1, 1)
        if self._replicated:
            # integrator state of ALL beads on every rank (they start from the same geometry); the force call reads the
            # rank's rows of it in place
            Ball = self.n_beads
            self._q_all = R.view(Bl, N, 3)[:1].repeat(Ball, 1, 1).contiguous()
            self._p_all = torch.zeros(Ball, N, 3, device=dev)
            self._f_all = torch.zeros(Ball, N, 3, device=dev)
            self.full = MDState(self._q_all, self._p_all, m, self._f_all)
            lo = self._lo
            self.state = MDState(self._q_all[lo:lo + Bl], self._p_all[lo:lo + Bl], m, self._f_all[lo:lo + Bl])
            nb = Ball
        else:
            self.state = MDState(R.view(Bl, N, 3), torch.zeros(Bl, N, 3, device=dev), m)
            nb = Bl
        self.integrator = self._rp
        self._m_rep = m.reshape(-1).repeat(Bl).contiguous()
        self._qt = torch.empty(nb, N, 3, device=dev)
        self._pt = torch.empty(nb, N, 3, device=dev)
        self._A = self._rp.A.to(dev)
        if self._dist and not self._replicated:
            self._pack = torch.empty(2, Bl, N, 3, device=dev)                    # (q, p) of the rank, one message
            self._gath = torch.empty(self._world, 2, Bl, N, 3, device=dev)
            self._pgath = torch.empty(self._world, Bl, N, 3, device=dev)
        self._meter = None                       # centroid observables: built by the first call that asks for one
        if self.thermostat is not None:          # NVT: the thermostat at step begin and end (md/simulator.py:126-150)
            if not getattr(self.thermostat, "ring_polymer", False) or not hasattr(self.thermostat, "apply_beads"):
                raise ValueError("RPMDSimulation needs a ring-polymer thermostat (PILELocalThermostat, PILEGlobalThermostat, TRPMDThermostat, "
                                 "NHCRingPolymerThermostat), got %s" % type(self.thermostat).__name__)
            self.thermostat.init(self._rp, self._idx_m1, self._n_atoms1)
            self._stepc = torch.zeros(1, dtype=torch.int64, device=dev)      # step counter on the device: fresh noise per graph replay
            # chain state and workspaces once, before the first capture; re-captured graphs point at the same tensors
            self.thermostat.prepare(torch.empty(self.n_beads, N, 3, device=dev), m)

    def _force_buffer(self, f):
        if not self._replicated:
            return super()._force_buffer(f)
        buf = self.state.forces.view(-1, 3)        # the rank's rows of the all-bead force tensor, written in place
        buf.copy_(f)
        return buf

    # -- the one collective primitive ------------------------------------------------------------
    def _all_gather(self, out: torch.Tensor, local: torch.Tensor):
        """``out[r] = local of rank r`` (contiguous buffers).  RCCL directly on the device buffers; other back-ends (gloo in
        the tests: it has no device all-gather) through pinned host staging."""
        import torch.distributed as dist
        self.n_collectives += 1
        if dist.get_backend(self.group) == "nccl":
            dist.all_gather_into_tensor(out.view(-1), local.view(-1), group=self.group)
            return
        h_out = torch.empty(out.shape, dtype=out.dtype)
        dist.all_gather_into_tensor(h_out.view(-1), local.detach().cpu().view(-1), group=self.group)
        out.copy_(h_out)

    # -- pieces of a step --------------------------------------------------------------------------
    def _thermostat(self, which):
        th = self.thermostat
        if self._replicated:                       # all beads, every rank, same counter-based noise / chain arithmetic: no exchange
            st, p_all, lo, n_local = self.full, self.full.momenta, 0, self.n_beads
        elif self._dist:                      # the rank's beads from everybody's momenta: ONE all-gather
            st = self.state
            self._all_gather(self._pgath, st.momenta)
            p_all, lo, n_local = self._pgath.view(self.n_beads, self._n1, 3), self._lo, self.n_local
        else:
            st, p_all, lo, n_local = self.state, self.state.momenta, 0, self.n_beads
        th.apply_beads(p_all, st.masses, lo, n_local, 0, self._stepc, which, self._pt)
        with torch.no_grad():
            st.momenta.copy_(self._pt)

    def _skin(self):
        thr = max(0.5 * self.nl.cutoff_shell - self.margin, 0.0)
        ref = None if self._complete else self.nl.previous_positions       # complete lists: nothing to watch
        return ref, thr, (None if self._complete else self.flag)

    def _mix(self):
        """kick + ring-polymer main step of the beads this rank integrates (skin test on the beads of its list)."""
        ref, thr, flag = self._skin()
        if self._replicated:
            st = self.full
            self.integrator.half_step(st)
            _ring_polymer_hip(st.positions, st.momenta, st.masses, self._A, 0, self.n_beads, self._qt, self._pt)
            with torch.no_grad():
                st.positions.copy_(self._qt)
                st.momenta.copy_(self._pt)
            if ref is not None:                    # skin criterion of the rank's own beads (a drift of zero length: test only)
                loc = self.state
                with torch.cuda.device(loc.positions.device):
                    check(lib().spk_md_kick_drift_f32(fptr(loc.positions), fptr(loc.momenta), None, fptr(self._m_rep), 0.0,
                                                      loc.positions.numel() // 3, fptr(ref), float(thr) ** 2,
                                                      _lib.iptr(flag, torch.int32), stream()))
            return
        st = self.state
        self.integrator.half_step(st)
        if self._dist:
            with torch.no_grad():
                self._pack[0].copy_(st.positions)
                self._pack[1].copy_(st.momenta)
            self._all_gather(self._gath, self._pack)
            q_all = self._gath[:, 0].reshape(self.n_beads, self._n1, 3)          # [world, n_local] -> beads (copy: strided)
            p_all = self._gath[:, 1].reshape(self.n_beads, self._n1, 3)
        else:
            q_all, p_all = st.positions, st.momenta
        _ring_polymer_hip(q_all, p_all, st.masses, self._A, self._lo, self.n_local, self._qt, self._pt, ref, thr, flag)
        with torch.no_grad():
            st.positions.copy_(self._qt)
            st.momenta.copy_(self._pt)

    def _finish(self):
        """forces of the new positions -> second kick (-> thermostat, step counter)."""
        if self._replicated:
            self._all_gather(self._f_all.view(self._world, -1), self.state.forces)
            self.integrator.half_step(self.full)
        else:
            self.integrator.half_step(self.state)
        if self.thermostat is not None:
            self._thermostat(1)
            with torch.no_grad():
                self._stepc.add_(1)

    def _step_body(self):
        """single process: the whole step (one graph).  Bead-parallel: only the force evaluation (the graph segment between
        the collectives); ``_one_step`` adds the rest."""
        if self._dist:
            self._force_eval()
            return
        if self.thermostat is not None:
            self._thermostat(0)
        self._mix()
        self._force_eval()
        self._finish()

    def _one_step(self):
        if not self._dist:
            return super()._one_step()
        if self.thermostat is not None:
            self._thermostat(0)
        self._mix()
        super()._one_step()                        # force call of the rank's beads: graph replay
        self._finish()

    @property
    def collectives_per_step(self) -> int:
        if not self._dist:
            return 0
        if self._replicated:
            return 1
        return 1 + (2 if self.thermostat is not None else 0)

    def _all_momenta(self):
        if self._replicated:
            return self.full.momenta
        if self._dist:
            raise NotImplementedError("centroid observables of exchange='state' over several ranks need the other ranks' beads")
        return self.state.momenta

    def _centroid_meter(self):
        if self._meter is None:
            kb = getattr(self.thermostat, "kb", KB_MD)
            self._meter = _RingPolymerThermostat(0.0, 1.0, kb=kb).init(self._rp, self._idx_m1, self._n_atoms1)
        return self._meter

    def centroid_kinetic_energy(self) -> torch.Tensor:
        """Kinetic energy of the centroid per molecule, [n_molecules] (``System.centroid_kinetic_energy``, md/system.py:523-537):
        the centroid momentum is the bead mean, p_c / sqrt(n_beads) of the normal-mode centroid ``spk_md_rp_centroid_f32`` writes.
        Needs the momenta of all beads on this process: single process or ``exchange="forces"``; with ``exchange="state"`` over
        several ranks it raises NotImplementedError (no collective is spent on an observable)."""
        return 0.5 * self._centroid_meter().centroid_kinetic2(self._all_momenta(), self.state.masses) / self.n_beads

    def centroid_temperature(self) -> torch.Tensor:
        """Instantaneous centroid temperature per molecule, [n_molecules] (md/system.py:539-555); 0 for a molecule without atoms.
        Same limit as ``centroid_kinetic_energy``."""
        ke = self.centroid_kinetic_energy()
        n = self._meter._n_atoms_mol.to(ke.dtype)
        return torch.where(n > 0, 2.0 * ke / (3.0 * n.clamp_min(1.0) * self._meter.kb), torch.zeros_like(ke))

    def spring_energy(self):
        """Spring energy of the beads this process holds (all of them unless ``exchange="state"`` over several ranks, where
        the links to the neighbouring ranks' beads are not visible locally)."""
        st = self.full if self._replicated else self.state
        q, m = st.positions, st.masses.reshape(1, -1, 1)
        d = q - torch.roll(q, -1, 0)
        return 0.5 * self._rp.omega ** 2 * (m * d * d).sum()

    def total_energy(self):
        return float(self.energy.sum() + self.kinetic_energy() + self.spring_energy())
