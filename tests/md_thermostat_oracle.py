"""Float64 restatement of the reference's classical thermostats (md/simulation_hooks/thermostats.py) and of the per-molecule
kinetic energy / temperature of md/system.py.  TEST INFRASTRUCTURE ONLY: plain torch, every function citing the reference lines
it restates; pinned to tests/golden/md_thermostat.npz (arrays the reference's own lifted methods computed,
tests/make_md_thermostat_golden.py) by tests/test_md_thermostat_reference.py.  The GPU tests use it for shapes the fixture does
not hold.  ``HostCompute`` / ``host_pile`` are host stand-ins for the device entries, so that the host classes of
``schnetpack_amd.md`` run without a GPU (the pattern of tests/cpu_reference_kernels.py).

Layout everywhere: momenta p [n_replicas, n_atoms, 3], masses [n_atoms], idx_m [n_atoms] ascending, n_atoms_mol [n_mol].
"""
import math

import torch

Tensor = torch.Tensor

# md/utils/thermostat_utils.py:18-44 (Yoshida-Suzuki weights); order 1 is the unsplit step, which the reference does not list
YS = {1: [1.0],
      3: [1.35120719195966, -1.70241438391932, 1.35120719195966],
      5: [0.41449077179438, 0.41449077179438, -0.65796308717750, 0.41449077179438, 0.41449077179438],
      7: [0.78451361047756, 0.23557321335936, -1.17767998417887, 1.31518632068390, -1.17767998417887, 0.23557321335936, 0.78451361047756]}


def sub_steps(dt: float, multi_step: int, order: int) -> Tensor:
    """thermostats.py:332-341."""
    return dt * torch.tensor(YS[order], dtype=torch.float64) / multi_step


def sum_atoms(x: Tensor, idx_m: Tensor, n_mol: int) -> Tensor:
    """system.py:217-231: x [R, N, ...] -> [R, n_mol, ...]."""
    out = torch.zeros((x.shape[0], n_mol) + tuple(x.shape[2:]), dtype=x.dtype)
    return out.index_add(1, idx_m, x)


def kinetic_energy2(p: Tensor, masses: Tensor, idx_m: Tensor, n_mol: int) -> Tensor:
    """2 x system.py:374-386: sum over the atoms of a molecule of |p|^2 / m, [R, n_mol]."""
    return sum_atoms((p ** 2).sum(2) / masses[None, :], idx_m, n_mol)


def temperature(ke2: Tensor, n_atoms_mol: Tensor, kB: float) -> Tensor:
    """system.py:407-421: 2 / (3 n kB) E_kin.  The reference multiplies the INTEGER atom counts by python floats, so the factor
    2 / (3 n kB) is a float32 number whatever the dtype of the system; restated as such."""
    factor = 2.0 / (3.0 * n_atoms_mol[None, :].to(torch.float32) * kB)
    return factor.to(ke2.dtype) * (0.5 * ke2)


def nhc_masses(dof: Tensor, kT: float, frequency: float, chain_length: int) -> Tensor:
    """thermostats.py:375-396: [..., L]; innermost dof kT / w^2, the rest kT / w^2."""
    m = torch.ones(tuple(dof.shape) + (chain_length,), dtype=dof.dtype)
    m[..., 0] = dof * kT / frequency ** 2
    m[..., 1:] = kT / frequency ** 2
    return m


def nhc_propagate(ke: Tensor, dof: Tensor, kT: float, m: Tensor, v: Tensor, f: Tensor, steps: Tensor, multi_step: int) -> Tensor:
    """thermostats.py:398-468 on chain state v, f, m [..., L] (v and f updated in place); returns the scaling factor [...]."""
    L = v.shape[-1]
    f[..., 0] = (ke - dof * kT) / m[..., 0]
    s = torch.ones_like(ke)
    for _ in range(multi_step):
        for ts in steps.tolist():
            v[..., -1] += 0.25 * f[..., -1] * ts
            for c in range(L - 2, -1, -1):
                co = torch.exp(-0.125 * ts * v[..., c + 1])
                v[..., c] = v[..., c] * co ** 2 + 0.25 * f[..., c] * co * ts
            s = s * torch.exp(-0.5 * ts * v[..., 0])
            f[..., 0] = (s * s * ke - dof * kT) / m[..., 0]
            for c in range(L - 1):
                co = torch.exp(-0.125 * ts * v[..., c + 1])
                v[..., c] = v[..., c] * co ** 2 + 0.25 * f[..., c] * co * ts
                f[..., c + 1] = (m[..., c] * v[..., c] ** 2 - kT) / m[..., c + 1]
            v[..., -1] += 0.25 * f[..., -1] * ts
    return s


def nhc_apply_global(p, masses, idx_m, n_atoms_mol, kT, frequency, v, f, steps, multi_step, m=None):
    """thermostats.py:491-511, global form.  v, f [R, n_mol, L] in place; returns (p', scale [R, n_mol]).  A molecule without atoms
    keeps its chain and has scale 1 (the project's rule; the reference never meets one).  ``m``: thermostat masses [R, n_mol, L]
    when they are not to be derived from kT and the frequency (the reference forms them from float32 buffers)."""
    n_mol = int(n_atoms_mol.shape[0])
    L = v.shape[-1]
    ke = kinetic_energy2(p, masses, idx_m, n_mol)
    dof = (3 * n_atoms_mol[None, :]).to(p.dtype).expand_as(ke)
    live = n_atoms_mol > 0
    s = torch.ones_like(ke)
    if bool(live.any()):
        vl, fl = v[:, live].clone(), f[:, live].clone()
        ml = nhc_masses(dof[:, live], kT, frequency, L) if m is None else m[:, live]
        s[:, live] = nhc_propagate(ke[:, live], dof[:, live], kT, ml, vl, fl, steps, multi_step)
        v[:, live], f[:, live] = vl, fl
    return p * s[:, idx_m, None], s


def nhc_apply_massive(p, masses, kT, frequency, v, f, steps, multi_step, m=None):
    """thermostats.py:483-487, :491-511, massive form.  v, f [R, N, 3, L] in place; returns p'.  ``m`` as in ``nhc_apply_global``."""
    ke = p ** 2 / masses[None, :, None]
    dof = torch.ones_like(p)
    s = nhc_propagate(ke, dof, kT, nhc_masses(dof, kT, frequency, v.shape[-1]) if m is None else m, v, f, steps, multi_step)
    return p * s


def berendsen_scale(ke2, n_atoms_mol, dt, tau, T0, kB):
    """thermostats.py:181-186; 1 where the molecule has no atoms or no kinetic energy (documented deviation: NaN there)."""
    T = temperature(ke2, n_atoms_mol.clamp_min(1), kB)
    ok = (n_atoms_mol[None, :] > 0) & (ke2 > 0)
    s = torch.sqrt(1.0 + dt / tau * (T0 / torch.where(ok, T, torch.ones_like(T)) - 1.0))
    return torch.where(ok, s, torch.ones_like(s))


def berendsen_apply(p, masses, idx_m, n_atoms_mol, dt, tau, T0, kB):
    """thermostats.py:172-189; returns (p', scale)."""
    s = berendsen_scale(kinetic_energy2(p, masses, idx_m, int(n_atoms_mol.shape[0])), n_atoms_mol, dt, tau, T0, kB)
    return p * s[:, idx_m, None], s


def langevin_coefficients(dt: float, tau: float):
    """thermostats.py:226-237."""
    c1 = math.exp(-0.5 * dt / tau)
    return c1, math.sqrt(1.0 - c1 ** 2)


def langevin_apply(p, masses, c1, c2, kB_T, xi):
    """thermostats.py:252-261 with the noise given: c1 p + sqrt(m kB T) c2 xi."""
    return c1 * p + torch.sqrt(masses[None, :, None] * kB_T) * c2 * xi


def half_step(p, F, dt):
    """md/integrators.py:59-70."""
    return p + 0.5 * F * dt


def main_step(R, p, masses, dt):
    """md/integrators.py:97-110."""
    return R + dt * p / masses[None, :, None]


# ------------------------------------------------------------------------------------------------ host stand-ins for the device entries
class HostCompute:
    """``compute_fn`` of BerendsenThermostat / NHCThermostat on host tensors (any float dtype), in place like the device entries."""

    @staticmethod
    def workspace(n_rep, n_atoms, n_mol, device):
        return torch.empty(1, dtype=torch.int32)

    @staticmethod
    def kinetic(p, masses, idx_m, n_mol, ke2, err, ws):
        ke2.copy_(kinetic_energy2(p, masses, idx_m, n_mol).reshape(-1))

    @staticmethod
    def nhc_global(ke2, n_atoms_mol, n_rep, L, multi_step, order, steps, kT, link_mass, vel, frc, scale):
        n_mol = int(n_atoms_mol.shape[0])
        ke = ke2.view(n_rep, n_mol)
        dof = (3 * n_atoms_mol[None, :]).to(ke.dtype).expand_as(ke)
        live = n_atoms_mol > 0
        v, f = vel.view(n_rep, n_mol, L), frc.view(n_rep, n_mol, L)
        s = torch.ones_like(ke)
        m = torch.full((n_rep, n_mol, L), link_mass, dtype=ke.dtype)
        m[..., 0] = dof * link_mass
        vl, fl = v[:, live].clone(), f[:, live].clone()
        s[:, live] = nhc_propagate(ke[:, live], dof[:, live], kT, m[:, live], vl, fl, torch.tensor(steps, dtype=ke.dtype), multi_step)
        v[:, live], f[:, live] = vl, fl
        scale.copy_(s.reshape(-1))

    @staticmethod
    def nhc_massive(p, masses, L, multi_step, order, steps, kT, link_mass, vel, frc):
        v, f = vel.t().reshape(tuple(p.shape) + (L,)).clone(), frc.t().reshape(tuple(p.shape) + (L,)).clone()
        ke = p ** 2 / masses[None, :, None]
        dof = torch.ones_like(p)
        m = torch.full(tuple(p.shape) + (L,), link_mass, dtype=p.dtype)
        s = nhc_propagate(ke, dof, kT, m, v, f, torch.tensor(steps, dtype=p.dtype), multi_step)
        p.mul_(s)
        vel.copy_(v.reshape(-1, L).t())
        frc.copy_(f.reshape(-1, L).t())

    @staticmethod
    def berendsen_scale(ke2, n_atoms_mol, n_rep, dt_over_tau, T0, kB, scale):
        scale.copy_(berendsen_scale(ke2.view(n_rep, -1), n_atoms_mol, dt_over_tau, 1.0, T0, kB).reshape(-1))

    @staticmethod
    def scale_molecules(p, scale, idx_m, n_mol, err):
        p.mul_(scale.view(p.shape[0], n_mol)[:, idx_m, None])


def host_pile(noise_fn):
    """``compute_fn`` of LangevinThermostat / PILELocalThermostat on the host: p' = M1 p + sqrt(m) noise_scale M2 xi with
    xi = noise_fn(n_beads, n_atoms, seed, step, which) -- what ``k_md_pile`` evaluates."""
    def pile(p_all, masses, M, noise_scale, seed, step, step_dev, which, bead0, n_local, p_out=None):
        B, n = int(p_all.shape[0]), int(p_all.shape[1])
        if step_dev is not None:
            step = int(step_dev.item())
        xi = noise_fn(B, n, seed, step, which).to(p_all.dtype)
        M = M.to(p_all.dtype)
        m = masses.reshape(1, -1, 1).to(p_all.dtype)
        out = (M[0] @ p_all.reshape(B, -1) + M[1] @ (m.sqrt() * noise_scale * xi).reshape(B, -1)).view(B, n, 3)[bead0:bead0 + n_local]
        if p_out is None:
            return out
        p_out.copy_(out)
        return p_out
    return pile


# ------------------------------------------------------------------------------------------------ the tolerance rule
U23 = 2.0 ** -23          # one float32 ulp of a number in [1, 2)


def allowed_error(ref64: Tensor, ref32: Tensor) -> float:
    """What a float32 evaluation may differ by from the reference's float64 result (absolute, per compared array): 4 x the
    reference's OWN float32-versus-float64 gap on the same case, and never less than 4 float32 ulp of the array's magnitude
    (the rule of the PILE coefficients and trajectories)."""
    ref64, ref32 = ref64.double(), ref32.double()
    return max(4.0 * float((ref32 - ref64).abs().max()), 4.0 * U23 * float(ref64.abs().max()))


def ke2_bound(p: Tensor, masses: Tensor, idx_m: Tensor, n_atoms_mol: Tensor) -> Tensor:
    """Round-off bound of a float32 sum of the n terms |p_a|^2 / m_a of a molecule against the exact sum of the same float32
    inputs, [R, n_mol]: (n + 4) 2^-24 sum|terms| -- n 2^-24 sum|terms| for the additions in any order, and 4 roundings for forming
    a term (two products folded into the third, the sum, the division)."""
    s = kinetic_energy2(p.double(), masses.double(), idx_m, int(n_atoms_mol.shape[0]))
    return (n_atoms_mol[None, :].double() + 4.0) * 2.0 ** -24 * s
