"""Float64 restatement of the point-charge electrostatics (atomistic/electrostatic.py), written from the formulas and independent of both the
module mirrors and the reference's code: pair sums with the pair functions of csrc/spk_coulomb.hip, and the reciprocal-space Ewald sum with
complex structure factors.  ``tests/test_electrostatic_reference.py`` pins it to the fixture the reference's own code produced
(tests/golden/electrostatic_cases.npz, tests/make_electrostatic_golden.py); gradients come from autograd of these float64 formulas.

Fixture layout: case ``c`` stores its inputs as ``c/R``, ``c/q``, ``c/idx_i`` ... and every variant ``v`` of the case its settings and results as
``c/v/kind``, ``c/v/E``, ``c/v/F``, ``c/v/dEdq`` (``W``, ``E_real``, ``E_rec`` where they apply) and ``c/v/gap_*``.
"""
import math

import numpy as np
import torch

#: case -> variants (the same names in the fixture)
COULOMB = {"C1": ["plain", "plain_cut", "damped", "damped_cut"], "C2": ["plain", "damped_cut"], "C3": ["damped_cut"]}
EWALD = {"E1": ["k4"], "E2": ["k4", "k4_screened"], "E3": ["k1", "k2"], "E4": ["k9"]}
SWITCH = (1.0, 3.0)
CUTOFF = 6.0
MADELUNG_NACL = 1.7475646


def case_inputs(gold, case):
    pre = case + "/"
    return {k[len(pre):]: gold[k] for k in gold.files if k.startswith(pre) and "/" not in k[len(pre):]}


def variant(gold, case, var):
    pre = "%s/%s/" % (case, var)
    return {k[len(pre):]: gold[k] for k in gold.files if k.startswith(pre)}


def switch(d, on, off):
    x = (d - on) / (off - on)
    xs = x.clamp(1e-12, 1.0 - 1e-12)
    s = 1.0 / (1.0 + torch.exp(1.0 / (1.0 - xs) - 1.0 / xs))
    return torch.where(x <= 0, torch.ones_like(x), torch.where(x >= 1, torch.zeros_like(x), s))


def chi(d, kind, on=SWITCH[0], off=SWITCH[1], alpha=0.0, screened=False):
    if kind == 0:
        return 1.0 / d
    if kind == 1:
        s = switch(d, on, off)
        return s / torch.sqrt(d * d + 1.0) + (1.0 - s) / d
    c = torch.erfc(math.sqrt(alpha) * d) / d
    return c * (1.0 - switch(d, on, off)) if screened else c


def pair_energy(r_ij, q, idx_i, idx_j, idx_m, n_mol, ke, kind, rc=0.0, shift=0.0, alpha=0.0, screened=False):
    """E [n_mol] = 1/2 ke sum_pairs q_i q_j v(d)."""
    d = r_ij.norm(dim=1)
    v = chi(d, kind, alpha=alpha, screened=screened)
    if rc > 0:
        v = torch.where(d <= rc, (v - shift) ** 2 / v, torch.zeros_like(v))
    e = 0.5 * ke * q[idx_i] * q[idx_j] * v
    return torch.zeros(n_mol, dtype=r_ij.dtype).index_add(0, idx_m[idx_i], e)


def kvecs(k_max):
    """The reference's integer vectors in its order: cartesian product of (0, 1 .. k_max, -1 .. -k_max), 0 < |n|^2 <= k_max^2 + 2."""
    rng = list(range(0, k_max + 1)) + [-k for k in range(1, k_max + 1)]
    return np.asarray([(a, b, c) for a in rng for b in rng for c in rng if 0 < a * a + b * b + c * c <= k_max * k_max + 2], dtype=np.float64)


def recip_energy(R, q, cell, idx_m, n_mol, ke, alpha, k_max):
    """E_rec [n_mol] with complex structure factors."""
    n = torch.tensor(kvecs(k_max), dtype=R.dtype)
    out = []
    for m in range(n_mol):
        sel = idx_m == m
        C = cell[m]
        k = 2.0 * math.pi * n @ torch.linalg.inv(C).T
        k2 = (k * k).sum(1)
        ph = R[sel] @ k.T
        S = torch.complex(q[sel, None] * torch.cos(ph), q[sel, None] * torch.sin(ph)).sum(0)
        V = torch.abs(torch.linalg.det(C))
        out.append(ke * (2.0 * math.pi / V * (torch.exp(-k2 / (4.0 * alpha)) / k2 * (S.real ** 2 + S.imag ** 2)).sum()
                         - math.sqrt(alpha / math.pi) * (q[sel] ** 2).sum()))
    return torch.stack(out)


def tensors(c, dtype=torch.float64):
    """The inputs of a case as torch tensors (R and q require grad)."""
    t = {k: torch.tensor(c[k], dtype=dtype if c[k].dtype.kind == "f" else torch.long) for k in ("R", "q", "cell", "offsets", "idx_i", "idx_j", "idx_m")}
    t["R"].requires_grad_()
    t["q"].requires_grad_()
    t["n_mol"] = int(c["n_mol"])
    return t


def coulomb_case(c, v):
    """(E, F, dEdq) of an EnergyCoulomb variant from this file's formulas."""
    t = tensors(c)
    r = t["R"][t["idx_j"]] - t["R"][t["idx_i"]] + t["offsets"]
    E = pair_energy(r, t["q"], t["idx_i"], t["idx_j"], t["idx_m"], t["n_mol"], float(v["ke"]), int(v["kind"]), float(v["rc"]), float(v["shift"]))
    gR, gq = torch.autograd.grad(E.sum(), [t["R"], t["q"]])
    return E.detach().numpy(), -gR.numpy(), gq.numpy()


def ewald_case(c, v):
    """(E, F, dEdq, E_real, E_rec) of an EnergyEwald variant from this file's formulas."""
    t = tensors(c)
    r = t["R"][t["idx_j"]] - t["R"][t["idx_i"]] + t["offsets"]
    ke, alpha = float(v["ke"]), float(v["alpha"])
    Er = pair_energy(r, t["q"], t["idx_i"], t["idx_j"], t["idx_m"], t["n_mol"], ke, 2, alpha=alpha, screened=bool(v["screened"]))
    Ek = recip_energy(t["R"], t["q"], t["cell"], t["idx_m"], t["n_mol"], ke, alpha, int(v["k_max"]))
    E = Er + Ek
    gR, gq = torch.autograd.grad(E.sum(), [t["R"], t["q"]])
    return E.detach().numpy(), -gR.numpy(), gq.numpy(), Er.detach().numpy(), Ek.detach().numpy()


def params8(v):
    """The parameter block of ``spk_coulomb_fwd_f32`` for a variant."""
    if "alpha" in v:
        return [float(v["ke"]), 2.0, 0.0, 0.0, SWITCH[0], SWITCH[1], float(v["alpha"]), float(bool(v["screened"]))]
    return [float(v["ke"]), float(int(v["kind"])), float(v["rc"]), float(v["shift"]), SWITCH[0], SWITCH[1], 0.0, 0.0]
