"""Float64 restatement of the reference's ring-polymer thermostats beyond PILE-L (md/simulation_hooks/thermostats_rpmd.py):
``NHCRingPolymerThermostat`` (local and global centroid), ``PILEGlobalThermostat`` and ``TRPMDThermostat``.  TEST INFRASTRUCTURE
ONLY: plain torch on any float dtype, every function citing the reference lines it restates; pinned to
tests/golden/md_rp_thermostat.npz (arrays the reference's own lifted methods computed, tests/make_md_rp_thermostat_golden.py) by
tests/test_md_rp_thermostat_reference.py.  The chain pass and the tolerance rule are those of tests/md_thermostat_oracle.py.

Layout: momenta p [n_beads, n_atoms, 3], masses [n_atoms], idx_m [n_atoms] ascending, n_atoms_mol [n_mol], C [n_beads, n_beads] the
normal-mode matrix (oracle/md_oracle.py), chain state v, f [n_beads, n_atoms, 3, chain_length] (the reference's).
"""
import torch

from md_thermostat_oracle import allowed_error, nhc_propagate, sum_atoms  # noqa: F401  (allowed_error: re-exported for the tests)

Tensor = torch.Tensor


# ------------------------------------------------------------------------------------------------ reading tests/golden/md_rp_thermostat.npz
def allowed_error_gap(ref64: Tensor, gap: float) -> float:
    """``allowed_error`` where the fixture stores of the reference's float32 run only its gap max |float32 - float64|: 4 x that gap,
    and never less than ``allowed_error``'s own floor (4 float32 ulp of the array's magnitude: what it returns for a gap of zero)."""
    return max(4.0 * float(gap), allowed_error(ref64, ref64))


def fixture_nhc(g, tag: str, local: bool, key: str, k: int):
    """(float64 result of the reference, its float32 gap) of NHC-RP case ``tag`` after ``k`` applications; key "p" momenta [B, N, 3],
    "v" / "f" chain velocities / forces [B, N, 3, L].  The chain state of a ``local=False`` run is stored as what distinguishes it
    from the ``local=True`` run (tests/make_md_rp_thermostat_golden.py asserts both statements on the reference's output): the
    modes k >= 1 are the local run's, the centroid rows are the molecule chains [n_mol, L] broadcast over atoms and components."""
    import numpy as np
    T = lambda x: torch.from_numpy(np.asarray(x))         # noqa: E731
    apps = [int(a) for a in (g["applications"] if key == "p" else g["state_at"])]
    i = apps.index(k)
    name = "nhc_%s_%s" % (tag, "loc" if local or key != "p" else "glo")
    ref = T(g["%s_f64_%s" % (name, key)])[i].clone()
    if not local and key != "p":
        mol = T(g["nhc_%s_glo_f64_%sc" % (tag, key)])[i]
        ref[0] = mol[T(g["idx_m"])][:, None, :].expand(ref.shape[1], 3, ref.shape[3])
    ci = [str(c) for c in g["nhc_cases"]].index(tag)
    gap = float(g["nhc_gaps"][ci, 0 if local else 1, "pvf".index(key), [int(a) for a in g["applications"]].index(k)])
    return ref, gap


def fixture_pile(g, case: str, k: int) -> Tensor:
    """float64 momenta of the reference for PILE case ``case`` ("pg_b<B>", "pgs", "tr_b<B>") after ``k`` applications."""
    import numpy as np
    return torch.from_numpy(np.asarray(g[case + "_f64_p"]))[[int(a) for a in g["applications"]].index(k)]


def to_normal(x: Tensor, C: Tensor) -> Tensor:
    """md/utils/normal_model_transformation.py:70-83: C x over the bead axis."""
    return (C.to(x.dtype) @ x.reshape(x.shape[0], -1)).view(x.shape)


def to_beads(x: Tensor, C: Tensor) -> Tensor:
    """md/utils/normal_model_transformation.py:85-98: C^T x."""
    return (C.to(x.dtype).t() @ x.reshape(x.shape[0], -1)).view(x.shape)


def rp_nhc_frequencies(omega_normal: Tensor, frequency: float) -> Tensor:
    """thermostats_rpmd.py:430-433 on a COPY of the integrator's frequencies: centroid entry 0.5 x the thermostat frequency."""
    w = omega_normal.clone()
    w[0] = 0.5 * frequency
    return w


def rp_nhc_dof(n_beads: int, idx_m: Tensor, n_atoms_mol: Tensor, local: bool, dtype=torch.float64) -> Tensor:
    """thermostats.py:349-354 and thermostats_rpmd.py:446-455: ones [B, N, 3]; global: centroid row 3 n_atoms of the atom's molecule."""
    dof = torch.ones(n_beads, idx_m.shape[0], 3, dtype=dtype)
    if not local:
        dof[0] = (3 * n_atoms_mol[idx_m]).to(dtype)[:, None]
    return dof


def rp_nhc_masses(kT: float, frequencies: Tensor, dof: Tensor, chain_length: int) -> Tensor:
    """thermostats_rpmd.py:436-453: kT / omega_k^2 for every link, the innermost link of the global centroid x 3 n_atoms.  (For the
    local form dof = 1 everywhere, so "innermost x dof" is the same statement.)"""
    m = (kT / frequencies.to(dof.dtype) ** 2)[:, None, None, None].expand(tuple(dof.shape) + (chain_length,)).clone()
    m[..., 0] = m[..., 0] * dof
    return m


def rp_nhc_apply(p, masses, idx_m, n_atoms_mol, C, kT, m, v, f, steps, multi_step, local=True):
    """thermostats_rpmd.py:457-501: kinetic term p_nm^2 / mass per (mode, atom, component) -- global: the centroid row holds the
    molecule's whole centroid sum -- one chain pass (thermostats.py:398-468), momenta x factor, back to beads.  v, f in place.
    ``m``: thermostat masses [B, N, 3, L]; dof follows from ``local``."""
    B = p.shape[0]
    pn = to_normal(p, C)
    ke = pn ** 2 / masses[None, :, None]
    if not local:
        kc = sum_atoms(ke[0:1].sum(2, keepdim=True), idx_m, int(n_atoms_mol.shape[0]))          # [1, n_mol, 1]
        ke = ke.clone()
        ke[0] = kc[0][idx_m].expand(-1, 3)
    dof = rp_nhc_dof(B, idx_m, n_atoms_mol, local, p.dtype)
    s = nhc_propagate(ke, dof, kT, m, v, f, steps, multi_step)
    return to_beads(pn * s, C)


def pile_global_alpha(K: Tensor, S: Tensor, R1: Tensor, c: float, kT: float, n_atoms_mol: Tensor) -> Tensor:
    """thermostats_rpmd.py:175-197 per molecule; 1 where the molecule has no atoms or no centroid kinetic energy (documented
    deviation: the reference divides by zero)."""
    ok = (n_atoms_mol > 0) & (K > 0)
    Ks = torch.where(ok, K, torch.ones_like(K))
    g = (1.0 - c) * kT / Ks
    a2 = c + S * g + 2.0 * R1 * torch.sqrt(c * g)
    a = torch.sqrt(a2) * torch.sign(R1 + torch.sqrt(c / g))
    return torch.where(ok, a, torch.ones_like(a))


def first_atoms(n_atoms_mol: Tensor) -> Tensor:
    return torch.cumsum(n_atoms_mol, 0) - n_atoms_mol


def pile_global_apply(p, masses, idx_m, n_atoms_mol, C, c1, c2, kT, xi):
    """thermostats_rpmd.py:147-208 with the normal-mode noise xi [B, N, 3] given.  R1 of molecule m is the centroid noise of the x
    component of ITS first atom (the project's rule; the reference's [0, 0, 0] is that for a single molecule).  Returns (p', alpha)."""
    n_mol = int(n_atoms_mol.shape[0])
    pn = to_normal(p, C)
    c1, c2, xi = c1.to(p.dtype), c2.to(p.dtype), xi.to(p.dtype)
    K = sum_atoms((pn[0:1] ** 2 / masses[None, :, None]).sum(2), idx_m, n_mol)[0]
    S = sum_atoms((xi[0:1] ** 2).sum(2), idx_m, n_mol)[0]
    fa = first_atoms(n_atoms_mol).clamp_max(max(int(p.shape[1]) - 1, 0))
    R1 = xi[0, fa, 0]
    alpha = pile_global_alpha(K, S, R1, float(c1[0]), kT, n_atoms_mol)
    out = pn.clone()
    out[0] = alpha[idx_m][:, None] * pn[0]
    out[1:] = c1[1:, None, None] * pn[1:] + torch.sqrt(masses[None, :, None] * kT) * c2[1:, None, None] * xi[1:]
    return to_beads(out, C), alpha


def centroid_temperature(p, masses, idx_m, n_atoms_mol, kB):
    """md/system.py:498-555: bead-mean momentum, kinetic energy per molecule, 2 / (3 kB n) E; 0 for a molecule without atoms."""
    pc = p.mean(0, keepdim=True)
    ke = 0.5 * sum_atoms((pc ** 2).sum(2) / masses[None, :], idx_m, int(n_atoms_mol.shape[0]))[0]
    n = n_atoms_mol.to(p.dtype)
    return torch.where(n > 0, 2.0 * ke / (3.0 * kB * n.clamp_min(1.0)), torch.zeros_like(ke))
