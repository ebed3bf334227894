"""Float64 closed-form restatement of the ZBL repulsion (atomistic/nuclear_repulsion.py:70-108) and of its derivatives, in numpy:

    a_z = z^p,  a_ij = (a_zi + a_zj) s,  phi(d) = sum_k c_k exp(-a_ij alpha_k d),  e(d) = z_i z_j phi(d) f_c(d) / d
    E_atom[i] = 1/2 ke sum_{e: idx_i[e] = i} e(d_e),   E[m] = sum_{i in m} E_atom[i]
    g_e = dE/dr_e = 1/2 ke e'(d_e) r_e / d_e,   F_i = sum_{e: idx_i[e] = i} g_e - sum_{e: idx_j[e] = i} g_e,   W[m] = sum_{e in m} g_e r_e^T

``f_c`` is the cosine cutoff 0.5 (cos(pi d / rc) + 1) [d < rc] (rc = 0: no cutoff function, f_c = 1).  tests/test_zbl_reference.py pins this file
to the fixture the reference's own code produced (tests/golden/zbl_cases.npz) at 1e-12; the device tests use the fixture itself.
"""
import numpy as np

CASES = ["a", "b", "c", "d", "e_half", "e_shuf", "f", "g", "h"]


def softplus(x):
    return np.log1p(np.exp(np.asarray(x, dtype=np.float64)))


def effective(a_pow, a_div, exponents, coefficients):
    """(p, s, alpha[4], c[4]) from the stored (inverse-softplus) parameters; c L1-normalised."""
    c = softplus(coefficients)
    return float(softplus(a_pow)[0]), float(softplus(a_div)[0]), softplus(exponents), c / np.abs(c).sum()


def params12(ke, rc, a_pow, a_div, exponents, coefficients):
    p, s, al, c = effective(a_pow, a_div, exponents, coefficients)
    return np.concatenate([[float(ke), float(rc), p, s], al, c])


def pair_terms(prm, zi, zj, d):
    """e(d) and e'(d) for arrays of pairs."""
    ke, rc, p, s = prm[:4]
    al, c = prm[4:8], prm[8:12]
    zi, zj = zi.astype(np.float64), zj.astype(np.float64)
    a = (zi ** p + zj ** p) * s
    ex = np.exp(-a[:, None] * al[None, :] * d[:, None])
    phi = (c[None, :] * ex).sum(1)
    dphi = (-a[:, None] * al[None, :] * c[None, :] * ex).sum(1)
    if rc > 0:
        inside = d < rc
        fc = np.where(inside, 0.5 * (np.cos(np.pi * d / rc) + 1.0), 0.0)
        dfc = np.where(inside, -0.5 * np.pi / rc * np.sin(np.pi * d / rc), 0.0)
    else:
        fc, dfc = np.ones_like(d), np.zeros_like(d)
    zz = zi * zj
    e = zz * phi * fc / d
    de = zz * ((dphi * fc + phi * dfc) / d - phi * fc / d ** 2)
    return e, de


def evaluate(prm, Z, R, offsets, idx_i, idx_j, idx_m, n_mol):
    """E [n_mol], E_atom [N], F [N, 3] = -dE/dR, W [n_mol, 3, 3] = dE/dstrain, all float64."""
    Z, R, offsets = np.asarray(Z), np.asarray(R, dtype=np.float64), np.asarray(offsets, dtype=np.float64)
    N = Z.shape[0]
    r = R[idx_j] - R[idx_i] + offsets
    d = np.sqrt((r * r).sum(1))
    e, de = pair_terms(np.asarray(prm, dtype=np.float64), Z[idx_i], Z[idx_j], d)
    h = 0.5 * prm[0]
    E_atom = np.zeros(N)
    np.add.at(E_atom, idx_i, h * e)
    E = np.zeros(n_mol)
    np.add.at(E, idx_m, E_atom)
    g = (h * de / d)[:, None] * r
    F = np.zeros((N, 3))
    np.add.at(F, idx_i, g)
    np.add.at(F, idx_j, -g)
    W = np.zeros((n_mol, 3, 3))
    np.add.at(W, idx_m[idx_i], g[:, :, None] * r[:, None, :])
    return E, E_atom, F, W


def case_inputs(gold, tag):
    """The arrays of one fixture case as a dict (keys without the case prefix)."""
    pre = tag + "_"
    return {k[len(pre):]: gold[k] for k in gold.files if k.startswith(pre)}


def case_params12(c):
    return params12(c["ke"], c["rc"], c["a_pow"], c["a_div"], c["exponents"], c["coefficients"])
