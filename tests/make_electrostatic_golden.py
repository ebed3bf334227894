"""Generator of tests/golden/electrostatic_cases.npz (a plain script, not collected by pytest):

    python tests/make_electrostatic_golden.py

It lifts, with ``ast`` at run time, the reference's own ``CoulombPotential``, ``DampedCoulombPotential``, ``EnergyCoulomb``, ``EnergyEwaldError`` and
``EnergyEwald`` (atomistic/electrostatic.py), compiles them against the reference's own ``nn`` (``scatter_add``, ``SwitchFunction``; through
oracle/refshim.py) and a ``spk_units`` stand-in that returns the project's unit factors (``ase`` is not available), runs them behind the
reference's own ``Strain`` and ``PairwiseDistances`` and stores ONLY arrays: the inputs (lists included) and E, F = -dE/dR, dE/dq (W = dE/dstrain
for the periodic ``EnergyCoulomb`` case, E_real and E_rec for Ewald) from a float64 run.  ``gap_* = max|x32 - x64| / max|x64|`` is the reference's
own float32 gap on the case; the generator asserts that it is below a quarter of the device tolerance (1e-5) and stores it.  On the exact
rock-salt lattice (E1) the forces vanish by symmetry: their gap is taken relative to max|E| / a, the scale the tests use there.

Cases (tests/electrostatic_oracle.py names the variants):
  C1   clusters of 5, 17 and 70 atoms, list radius 7: rows of 16 and 17 entries (either side of the 16-lane group), a molecule across the 64-atom
       reduction chunk, pairs below switch_on = 1, inside the switch, beyond switch_off = 3 and beyond cutoff = 6, one charge 0;
       {plain, damped} x {no cutoff, shifted cutoff 6}
  C2   the same batch as a directed half list (i < j), shuffled: neither symmetric nor sorted
  C3   two periodic triclinic cells (6 and 9 atoms) with offsets, behind Strain: W
  E1   rock salt, 8 ions, a = 5.64, alpha = 0.1225, k_max = 4, list radius 12, ke = 1 (Madelung constant)
  E2   the cell jittered (sigma 0.25) and made triclinic (sigma 0.3), alpha = 0.16, k_max = 4, list radius 9, with and without SwitchFunction(1, 3)
  E3   three boxes of 63, 65 and 129 atoms (atom tile 64, slab 256: the last box spans two slabs), k_max = 1 (K = 26) and 2; one box is not neutral,
       one charge is 0, one atom sits outside its cell on both sides
  E4   geometry E2 with k_max = 9, one above the kernels' cap
"""
import ast
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim  # noqa: E402
from oracle.make_golden import save_npz_reproducible  # noqa: E402
from schnetpack_amd import units as project_units  # noqa: E402
import electrostatic_oracle as EO  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "electrostatic_cases.npz")
TOL = 1.0e-5
A_NACL = 5.64


def reference_classes():
    ns = refshim.load()
    path = os.path.join(refshim.REF_SRC, "schnetpack", "atomistic", "electrostatic.py")
    env = {"torch": torch, "nn": torch.nn, "np": np, "properties": ns.properties, "snn": ns.nn,
           "spk_units": types.SimpleNamespace(convert_units=project_units.convert_units)}
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.ClassDef):
            for fn in node.body:
                if isinstance(fn, ast.FunctionDef):
                    fn.returns = None
                    for a in fn.args.args + fn.args.kwonlyargs:
                        a.annotation = None
            exec(compile(ast.Module([node], []), "electrostatic.py", "exec"), env)
    return ns, types.SimpleNamespace(**{k: env[k] for k in ("CoulombPotential", "DampedCoulombPotential", "EnergyCoulomb", "EnergyEwald", "EnergyEwaldError")})


# ----------------------------------------------------------------------------------------------------------------- geometry
def neighbour_list(R, cell, pbc, cutoff):
    """Every directed pair (i, j, S) with |R_j - R_i + S cell| < cutoff, sorted by i (then j, then shift).  float64."""
    N = R.shape[0]
    nmax = np.ceil(cutoff * np.linalg.norm(np.linalg.inv(cell), axis=0)).astype(int) if pbc else np.zeros(3, dtype=int)
    sh = np.asarray([(a, b, c) for a in range(-nmax[0], nmax[0] + 1) for b in range(-nmax[1], nmax[1] + 1) for c in range(-nmax[2], nmax[2] + 1)],
                    dtype=np.float64)
    off = sh @ cell
    d = R[None, :, None, :] - R[:, None, None, :] + off[None, None, :, :]
    dist = np.linalg.norm(d, axis=-1)
    keep = dist < cutoff
    keep[np.arange(N), np.arange(N), np.nonzero((sh == 0).all(1))[0][0]] = False
    i, j, s = np.nonzero(keep)
    return i.astype(np.int64), j.astype(np.int64), off[s]


def place(rng, n, radius, dmin, centre):
    pts = []
    while len(pts) < n:
        p = rng.uniform(-radius, radius, 3)
        if np.linalg.norm(p) <= radius and all(np.linalg.norm(p - x) >= dmin for x in pts):
            pts.append(p)
    return np.asarray(pts) + np.asarray(centre)


def place_box(rng, n, cell, dmin):
    pts = []
    imgs = np.asarray([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], dtype=np.float64) @ cell
    while len(pts) < n:
        p = rng.uniform(0, 1, 3) @ cell
        if all(np.linalg.norm(p - x[None, :] + imgs, axis=1).min() >= dmin for x in pts):
            pts.append(p)
    return np.asarray(pts)


def batch(mols):
    """mols: list of (R, q, cell, pbc, list radius) -> one case dict."""
    R, q, cells, ii, jj, off, idx_m, n0 = [], [], [], [], [], [], [], 0
    for m, (r, c, cell, pbc, rad) in enumerate(mols):
        i, j, o = neighbour_list(r, cell, pbc, rad)
        R.append(r), q.append(c), cells.append(cell), ii.append(i + n0), jj.append(j + n0), off.append(o), idx_m.append(np.full(len(r), m, dtype=np.int64))
        n0 += len(r)
    return {"R": np.concatenate(R), "q": np.concatenate(q), "cell": np.stack(cells), "idx_i": np.concatenate(ii), "idx_j": np.concatenate(jj),
            "offsets": np.concatenate(off).reshape(-1, 3), "idx_m": np.concatenate(idx_m), "n_mol": np.int64(len(mols))}


def case_c1():
    big = np.eye(3) * 100.0
    for seed in range(100):
        rng = np.random.default_rng(4100 + seed)
        mols = [(place(rng, 5, 1.6, 0.8, (-17.0, 0.0, 0.0)), None), (place(rng, 17, 2.6, 0.8, (17.0, 0.0, 0.0)), None),
                (place(rng, 70, 7.0, 0.8, (0.0, 0.0, 0.0)), None)]
        c = batch([(r, rng.uniform(-1.0, 1.0, len(r)), big, False, 7.0) for r, _ in mols])
        c["q"][7] = 0.0
        rows = np.bincount(c["idx_i"], minlength=len(c["R"]))
        d = np.linalg.norm(c["R"][c["idx_j"]] - c["R"][c["idx_i"]], axis=1)
        if 16 in rows and 17 in rows and (d < 1.0).any() and ((d > 1.0) & (d < 3.0)).any() and (d > 6.0).any():
            return c
    raise RuntimeError("no seed gives rows of 16 and 17 entries")


def case_c2(c1):
    rng = np.random.default_rng(4200)
    keep = np.nonzero(c1["idx_i"] < c1["idx_j"])[0]
    keep = keep[rng.permutation(len(keep))]
    c = dict(c1)
    for k in ("idx_i", "idx_j", "offsets"):
        c[k] = c1[k][keep]
    return c


def case_c3():
    rng = np.random.default_rng(4300)
    mols = []
    for n, a in ((6, 7.0), (9, 8.0)):
        cell = np.eye(3) * a + rng.normal(0, 0.4, (3, 3))
        mols.append((place_box(rng, n, cell, 1.2), rng.uniform(-1.0, 1.0, n), cell, True, 7.0))
    return batch(mols)


def rock_salt():
    a = A_NACL
    na = np.asarray([(0, 0, 0), (1, 1, 0), (1, 0, 1), (0, 1, 1)], dtype=np.float64) * a / 2
    cl = np.asarray([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)], dtype=np.float64) * a / 2
    return np.concatenate([na, cl]), np.asarray([1.0] * 4 + [-1.0] * 4), np.eye(3) * a


def case_e1():
    R, q, cell = rock_salt()
    return batch([(R, q, cell, True, 12.0)])


def case_e2():
    rng = np.random.default_rng(4500)
    R, q, cell = rock_salt()
    return batch([(R + rng.normal(0, 0.25, R.shape), q, cell + rng.normal(0, 0.3, (3, 3)), True, 9.0)])


def case_e3():
    rng = np.random.default_rng(4600)
    mols = []
    for k, n in enumerate((63, 65, 129)):
        L = (n * 40.0) ** (1.0 / 3.0)
        cell = np.eye(3) * L + rng.normal(0, 0.3, (3, 3))
        R = place_box(rng, n, cell, 1.6)
        q = rng.uniform(-1.0, 1.0, n)
        q -= q.mean()
        if k == 1:
            q[3] += 0.7                      # this box is not neutral
        mols.append((R, q, cell, True, 5.0))
    mols[0][1][5] = 0.0
    mols[2][0][11] += -1.0 * mols[2][2][0] + 1.0 * mols[2][2][1]      # fractional coordinates below 0 on one axis and above 1 on another
    return batch(mols)


# ----------------------------------------------------------------------------------------------------------------- reference runs
def run(ns, module, c, dtype, strain):
    p = ns.properties
    t = lambda k: torch.tensor(c[k], dtype=dtype if c[k].dtype.kind == "f" else torch.long)
    inp = {p.R: t("R"), p.cell: t("cell"), p.offsets: t("offsets"), p.idx_i: t("idx_i"), p.idx_j: t("idx_j"), p.idx_m: t("idx_m"),
           p.partial_charges: t("q")}
    inp[p.R].requires_grad_()
    inp[p.partial_charges].requires_grad_()
    module = module.to(dtype)
    if strain:
        inp = ns.response.Strain()(inp)
    inp = ns.distances.PairwiseDistances()(inp)
    inp = module(inp)
    E = inp["e"]
    wrt = [inp[p.R], inp[p.partial_charges]] + ([inp[p.strain]] if strain else [])
    g = torch.autograd.grad(E.sum(), wrt)
    out = {"E": E.detach().double().numpy(), "F": -g[0].double().numpy(), "dEdq": g[1].double().numpy()}
    if strain:
        out["W"] = g[2].double().numpy()
    return out, inp


def gaps(x64, x32, scales=None):
    out = {}
    for k in x64:
        s = np.abs(x64[k]).max() if not (scales and k in scales) else scales[k]
        out["gap_" + k] = np.float64(np.abs(x32[k] - x64[k]).max() / (s if s > 0 else 1.0))
    return out


def main():
    ns, ref = reference_classes()
    SF = ns.nn.SwitchFunction
    arrs = {}
    c1 = case_c1()
    cases = {"C1": c1, "C2": case_c2(c1), "C3": case_c3(), "E1": case_e1(), "E2": case_e2(), "E3": case_e3()}
    cases["E4"] = cases["E2"]
    for tag, c in cases.items():
        for k, v in c.items():
            arrs["%s/%s" % (tag, k)] = v
        print("%s: %d atoms, %d pairs, rows %d..%d" % (tag, len(c["R"]), len(c["idx_i"]), np.bincount(c["idx_i"], minlength=len(c["R"])).min(),
                                                     np.bincount(c["idx_i"], minlength=len(c["R"])).max()))

    def store(tag, var, settings, x64, x32, scales=None):
        g = gaps(x64, x32, scales)
        for k, v in list(settings.items()) + list(x64.items()) + list(g.items()):
            arrs["%s/%s/%s" % (tag, var, k)] = np.asarray(v)
        print("  %s/%s: E %s  %s" % (tag, var, np.array2string(x64["E"], precision=6), " ".join("%s %.2e" % kv for kv in g.items())))
        assert all(v < TOL / 4 for v in g.values()), (tag, var, g)

    for tag, variants in EO.COULOMB.items():
        for var in variants:
            mk = lambda: ref.EnergyCoulomb("eV", "Ang", ref.DampedCoulombPotential(SF(*EO.SWITCH)) if var.startswith("damped") else ref.CoulombPotential(), "e",
                                           use_neighbors_lr=False, cutoff=EO.CUTOFF if var.endswith("_cut") else None)
            m = mk()
            settings = {"ke": np.float64(m.ke.double()[0]), "kind": np.int64(1 if var.startswith("damped") else 0),
                        "rc": np.float64(EO.CUTOFF if var.endswith("_cut") else 0.0),
                        "shift": np.float64(m.double().shift.reshape(-1)[0]) if var.endswith("_cut") else np.float64(0.0)}
            x64, _ = run(ns, mk(), cases[tag], torch.float64, tag == "C3")
            x32, _ = run(ns, mk(), cases[tag], torch.float32, tag == "C3")
            store(tag, var, settings, x64, x32)

    ew = {"E1": (0.1225, 1.0), "E2": (0.16, None), "E3": (0.16, None), "E4": (0.16, None)}
    for tag, variants in EO.EWALD.items():
        for var in variants:
            alpha, ke_unit = ew[tag]
            k_max = int(var[1])
            screened = var.endswith("_screened")
            # ke = 1 (E1): energy and position units are the atomic units the constant is defined in
            mk = lambda: ref.EnergyEwald(alpha, k_max, "Ha" if ke_unit else "eV", "Bohr" if ke_unit else "Ang", "e", use_neighbors_lr=False,
                                         screening_fn=SF(*EO.SWITCH) if screened else None)
            m = mk().double()
            settings = {"ke": np.float64(m.ke[0]), "alpha": np.float64(m.alpha[0]), "k_max": np.int64(k_max), "screened": np.int64(screened)}
            x64, inp = run(ns, m, cases[tag], torch.float64, False)
            p = ns.properties
            q, idx_m, n_mol = inp[p.partial_charges].detach(), inp[p.idx_m], int(cases[tag]["n_mol"])
            d = inp[p.Rij].detach().norm(dim=1)
            x64["E_real"] = m._real_space(q, d, inp[p.idx_i], inp[p.idx_j], idx_m, len(q), n_mol).detach().numpy()
            x64["E_rec"] = m._reciprocal_space(q, inp[p.R].detach(), inp[p.cell], idx_m, n_mol).detach().numpy()
            x32, _ = run(ns, mk(), cases[tag], torch.float32, False)
            x32["E_real"], x32["E_rec"] = x64["E_real"], x64["E_rec"]
            scales = {"F": np.abs(x64["E"]).max() / A_NACL} if tag == "E1" else None
            store(tag, var, settings, x64, x32, scales)
            if tag == "E1":
                print("  Madelung: %.8f" % (-x64["E"][0] * A_NACL / 8.0))
                assert abs(-x64["E"][0] * A_NACL / 8.0 / EO.MADELUNG_NACL - 1.0) < 1e-6

    # what the mirrors must reproduce of the reference's modules: state_dict keys, buffer shapes, the k-vectors
    mods = {"EnergyCoulomb": ref.EnergyCoulomb("eV", "Ang", ref.DampedCoulombPotential(SF(*EO.SWITCH)), "e", cutoff=EO.CUTOFF),
            "EnergyCoulombPlain": ref.EnergyCoulomb("eV", "Ang", ref.CoulombPotential(), "e", cutoff=EO.CUTOFF),
            "EnergyEwald": ref.EnergyEwald(0.16, 2, "eV", "Ang", "e", screening_fn=SF(*EO.SWITCH)), "SwitchFunction": SF(*EO.SWITCH)}
    for name, m in mods.items():
        sd = m.state_dict()
        arrs["ref/%s/keys" % name] = np.asarray(list(sd.keys()))
        arrs["ref/%s/shapes" % name] = np.asarray([",".join(str(s) for s in v.shape) for v in sd.values()])
    for km in (1, 2, 4):
        arrs["ref/kvecs_k%d" % km] = ref.EnergyEwald(0.16, km, "eV", "Ang", "e").kvecs.double().numpy()
    save_npz_reproducible(OUT, arrs)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(arrs), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
