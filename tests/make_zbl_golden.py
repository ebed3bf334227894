"""Generator of tests/golden/zbl_cases.npz (a plain script, not collected by pytest):

    python tests/make_zbl_golden.py

It lifts, with ``ast`` at run time, the reference's own ``ZBLRepulsionEnergy`` (``__init__`` / ``forward``, atomistic/nuclear_repulsion.py) and
``Aggregation`` (atomistic/aggregation.py), compiles them against the reference's own ``nn`` (``softplus_inverse``, ``scatter_add``,
``CosineCutoff``; through oracle/refshim.py) and a ``spk_units`` stand-in that returns the project's unit factors (schnetpack_amd/units.py:
``ase`` is not available), runs them behind the reference's own ``Strain`` and ``PairwiseDistances`` and stores ONLY arrays: the inputs, the unit
factors used, the stored parameters and E, E_atom, F = -dE/dR, W = dE/dstrain -- each once from a float64 and once from a float32 run.  The
difference ``gap_* = max|x32 - x64| / max|x64|`` is the reference's own float32 gap; the generator asserts it is below a quarter of the device
tolerance (1e-5) for every case and quantity, and stores it.

E_atom is not an output of the reference's module: it is the same lifted forward run with every atom as its own molecule.  The reference
sizes its output by ``int(idx_m[-1]) + 1``; case (b) declares one more, empty, molecule whose expected energy, zero, is appended here.

Cases (each the smallest at which its code path can go wrong):
  a       2 atoms, 1 pair, Z = 79 / 79, d = 0.3 A
  b       molecules of 1, 2, 5, 9 atoms, Z from {1, 6, 8, 79}, cutoff 5 A, n_mol = 5 (a trailing molecule without atoms)
  c       one cluster whose atoms have 1, 15, 16, 17, 33 and 65 neighbours (either side of a 16-lane sub-group, 2 x 16 and a wavefront)
  d       8 atoms in a triclinic periodic cell, cutoff above the cell heights: pairs with own images and several images of one neighbour
  e_half  list (b) delivered as a half list;  e_shuf  list (b) with its edges shuffled (neither sorted nor row-contiguous)
  f       geometry (b), list built at 1.3 x the ZBL radius (skin pairs)
  g       geometry (b), no cutoff function
  h       geometry (b), non-default parameters (coefficients that do not sum to 1), kcal/mol
"""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim  # noqa: E402
from oracle.make_golden import save_npz_reproducible  # noqa: E402
from schnetpack_amd import units as project_units  # noqa: E402
import zbl_oracle as ZO  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "zbl_cases.npz")
TOL = 1.0e-5                 # the device parity contract; the reference's own float32 gap must stay below TOL / 4
SEED = 20241


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


def reference_classes():
    import types
    ns = refshim.load()
    root = os.path.join(refshim.REF_SRC, "schnetpack", "atomistic")
    env = {"torch": torch, "nn": torch.nn, "F": torch.nn.functional, "properties": ns.properties, "snn": ns.nn,
           "spk_units": types.SimpleNamespace(convert_units=project_units.convert_units)}
    zbl = _lift_class(os.path.join(root, "nuclear_repulsion.py"), "ZBLRepulsionEnergy", env)
    agg = _lift_class(os.path.join(root, "aggregation.py"), "Aggregation", {"torch": torch, "nn": torch.nn})
    return ns, zbl, agg


# ----------------------------------------------------------------------------------------------------------------- geometry
def neighbour_list(R, cell, pbc, cutoff):
    """Every directed pair (i, j, S) with |R_j - R_i + S cell| < cutoff, sorted by i (then j, then shift).  float64."""
    N = R.shape[0]
    if pbc:
        inv = np.linalg.inv(cell)
        heights = 1.0 / np.linalg.norm(inv, axis=0)
        nmax = np.ceil(cutoff / heights).astype(int)
    else:
        nmax = np.zeros(3, dtype=int)
    shifts = [(a, b, c) for a in range(-nmax[0], nmax[0] + 1) for b in range(-nmax[1], nmax[1] + 1) for c in range(-nmax[2], nmax[2] + 1)]
    ii, jj, off = [], [], []
    for i in range(N):
        for j in range(N):
            for s in shifts:
                if i == j and s == (0, 0, 0):
                    continue
                o = np.asarray(s, dtype=np.float64) @ cell
                if np.linalg.norm(R[j] - R[i] + o) < cutoff:
                    ii.append(i), jj.append(j), off.append(o)
    return np.asarray(ii, dtype=np.int64), np.asarray(jj, dtype=np.int64), np.asarray(off, dtype=np.float64).reshape(-1, 3)


def place(rng, n, radius, dmin, centre=(0.0, 0.0, 0.0), images=None):
    """n points in a ball, no two closer than dmin (also to the periodic images of each other, if given)."""
    pts = []
    while len(pts) < n:
        p = rng.uniform(-radius, radius, 3)
        if np.linalg.norm(p) > radius:
            continue
        q = p + np.asarray(centre)
        others = [x + s for x in pts + [q] for s in (images if images is not None else [np.zeros(3)])]
        ok = all(np.linalg.norm(q - x) >= dmin for x in others if np.linalg.norm(q - x) > 0)
        if ok:
            pts.append(q)
    return np.asarray(pts)


BIG_CELL = np.eye(3) * 100.0


def geometry_b(rng, dmin):
    sizes = [1, 2, 5, 9]
    # centres 12 A apart (no pair between molecules even on the 6.5 A skin list) and close to the origin: the reference forms the virial
    # from R (x) dE/dR, whose float32 cancellation error grows with the coordinates
    centres = [(-6.0, -6.0, 0.0), (6.0, -6.0, 0.0), (-6.0, 6.0, 0.0), (6.0, 6.0, 0.0)]
    mols = [place(rng, n, {1: 1.1, 2: 1.3, 5: 1.9, 7: 2.0}[n], dmin, centre=centres[k]) for k, n in enumerate([1, 2, 5, 7])]
    # the two outermost atoms of the largest molecule are 5.7 A apart: inside the 6.5 A skin list of case f, outside the 5 A ZBL radius
    arm = np.asarray([2.15 + dmin, 0.0, 0.0])
    mols[3] = np.concatenate([mols[3], [np.asarray(centres[3]) + arm, np.asarray(centres[3]) - arm]])
    R = np.concatenate(mols)
    Z = rng.choice([1, 6, 8, 79], size=R.shape[0])
    Z[1], Z[2] = 79, 8
    idx_m = np.repeat(np.arange(len(sizes)), sizes)
    return dict(Z=Z.astype(np.int64), R=R, idx_m=idx_m.astype(np.int64), n_mol=5, cell=np.stack([BIG_CELL] * 5), pbc=False)


def geometry_c(rng, dmin):
    N = 66
    R = place(rng, N, 2.9 * max(1.0, dmin / 0.8), dmin)
    Z = rng.choice([1, 6, 8, 79], size=N).astype(np.int64)
    pairs = [(0, k) for k in range(1, N)]                                   # atom 0: 65 neighbours
    pairs += [(1, k) for k in range(5, 37)]                                 # atom 1: 1 + 32 = 33
    pairs += [(2, k) for k in range(37, 53)]                                # atom 2: 1 + 16 = 17
    pairs += [(3, k) for k in list(range(53, 65)) + [5, 6, 7]]              # atom 3: 1 + 15 = 16
    pairs += [(4, k) for k in range(8, 22)]                                 # atom 4: 1 + 14 = 15;  atom 65: the hub only = 1
    both = sorted(set(pairs + [(j, i) for i, j in pairs]))
    ii, jj = np.asarray([p[0] for p in both], dtype=np.int64), np.asarray([p[1] for p in both], dtype=np.int64)
    deg = np.bincount(ii, minlength=N)
    assert [deg[k] for k in (0, 1, 2, 3, 4, 65)] == [65, 33, 17, 16, 15, 1], deg
    return dict(Z=Z, R=R, idx_m=np.zeros(N, dtype=np.int64), n_mol=1, cell=BIG_CELL[None], pbc=False, idx_i=ii, idx_j=jj,
                offsets=np.zeros((ii.shape[0], 3)))


def geometry_d(rng, dmin):
    cell = np.array([[4.3, 0.0, 0.0], [1.1, 4.1, 0.0], [0.7, -0.9, 4.4]])
    images = [np.asarray([a - 1, b - 1, c - 1], dtype=np.float64) @ cell for a, b, c in np.ndindex(3, 3, 3)]
    frac = []
    while len(frac) < 8:
        f = rng.uniform(0, 1, 3)
        q = f @ cell
        if all(np.linalg.norm(q - (g @ cell) + s) >= dmin for g in frac for s in images):
            frac.append(f)
    R = np.asarray(frac) @ cell
    Z = np.asarray([79, 8, 1, 6, 8, 1, 79, 6], dtype=np.int64)
    return dict(Z=Z, R=R, idx_m=np.zeros(8, dtype=np.int64), n_mol=1, cell=cell[None], pbc=True)


# ----------------------------------------------------------------------------------------------------------------- reference runs
def run_reference(ns, zbl_cls, agg_cls, case, dtype):
    """E, E_atom, F, W of one case from the reference's own modules in ``dtype`` (+ the module, for its stored parameters)."""
    cut = ns.nn.CosineCutoff(case["rc"]) if case["rc"] > 0 else None
    mod = zbl_cls(case["energy_unit"], case["position_unit"], "e_zbl", trainable=True, cutoff_fn=cut)
    if case.get("raw") is not None:
        with torch.no_grad():
            for k, v in case["raw"].items():
                getattr(mod, k).copy_(torch.as_tensor(v, dtype=torch.float32))
    mod = mod.to(dtype)
    agg = agg_cls(["e_zbl", "e_other"], "energy")
    strain_mod, dist_mod = ns.response.Strain(), ns.distances.PairwiseDistances()
    P = ns.properties

    def once(idx_m, n_cells):
        R = torch.tensor(case["R"], dtype=dtype, requires_grad=True)
        cell = torch.tensor(case["cell"][:1].repeat(n_cells, 0) if n_cells != case["cell"].shape[0] else case["cell"], dtype=dtype)
        inp = {P.Z: torch.tensor(case["Z"]), P.R: R, P.cell: cell, P.offsets: torch.tensor(case["offsets"], dtype=dtype),
               P.idx_i: torch.tensor(case["idx_i"]), P.idx_j: torch.tensor(case["idx_j"]), P.idx_m: torch.tensor(idx_m)}
        inp = mod(dist_mod(strain_mod(inp)))
        return inp, R

    inp, R = once(case["idx_m"], case["cell"].shape[0])
    E = inp["e_zbl"]
    inp["e_other"] = torch.full_like(E, 2.5)
    total = agg(inp)["energy"]
    gR, gS = torch.autograd.grad(E.sum(), [R, inp[P.strain]])
    n_mol = case["n_mol"]
    pad = n_mol - E.shape[0]
    W = gS.detach().numpy()[: E.shape[0]]
    E_np = np.concatenate([E.detach().numpy(), np.zeros(pad, dtype=E.detach().numpy().dtype)])
    W_np = np.concatenate([W, np.zeros((pad, 3, 3), dtype=W.dtype)])
    agg_np = np.concatenate([total.detach().numpy(), np.full(pad, 2.5, dtype=E_np.dtype)])
    N = case["Z"].shape[0]
    per_atom, _ = once(np.arange(N, dtype=np.int64), N)
    return dict(E=E_np, E_atom=per_atom["e_zbl"].detach().numpy(), F=-gR.detach().numpy(), W=W_np, agg=agg_np), mod


def gap(x32, x64):
    scale = np.abs(x64).max()
    return float(np.abs(x32.astype(np.float64) - x64).max() / scale) if scale > 0 else float(np.abs(x32).max())


def build_cases(dmin):
    rng = np.random.default_rng(SEED)
    cases = {}
    base = dict(energy_unit="eV", position_unit="Ang", rc=5.0, raw=None)
    a = dict(base, Z=np.asarray([79, 79], dtype=np.int64), R=np.asarray([[0.1, 0.2, -0.1], [0.1 + 0.3 * 2 / 3, 0.2 + 0.3 * 2 / 3, -0.1 + 0.3 / 3]]),
             idx_m=np.zeros(2, dtype=np.int64), n_mol=1, cell=BIG_CELL[None], pbc=False)
    cases["a"] = a
    gb = geometry_b(rng, dmin)
    cases["b"] = dict(base, **gb)
    cases["c"] = dict(base, **geometry_c(rng, dmin))
    cases["c"]["rc"] = 6.0 * max(1.0, dmin / 0.8)              # every chosen pair inside the radius
    cases["d"] = dict(base, **geometry_d(rng, max(dmin, 1.0)))
    cases["f"] = dict(base, list_cutoff=6.5, **gb)
    cases["g"] = dict(base, **gb)
    cases["g"]["rc"], cases["g"]["list_cutoff"] = 0.0, 5.0
    raw = dict(a_pow=[-1.1], a_div=[1.7], exponents=[2.9, 1.2, -0.4, -1.5], coefficients=[-1.0, 0.3, -0.6, -2.5])
    cases["h"] = dict(base, **gb)
    cases["h"].update(raw=raw, energy_unit="kcal/mol", rc=4.0, list_cutoff=5.0)
    for tag, c in cases.items():
        if "idx_i" not in c:
            c["idx_i"], c["idx_j"], c["offsets"] = neighbour_list(c["R"], c["cell"][0], c["pbc"], c.get("list_cutoff", c["rc"]))
    b = cases["b"]
    assert cases["f"]["idx_i"].shape[0] > b["idx_i"].shape[0], "case f needs pairs between the ZBL radius and the list cutoff"
    keep = b["idx_i"] < b["idx_j"]
    cases["e_half"] = dict(b, idx_i=b["idx_i"][keep], idx_j=b["idx_j"][keep], offsets=b["offsets"][keep])
    perm = rng.permutation(b["idx_i"].shape[0])
    cases["e_shuf"] = dict(b, idx_i=b["idx_i"][perm], idx_j=b["idx_j"][perm], offsets=b["offsets"][perm])
    return cases


def main():
    ns, zbl_cls, agg_cls = reference_classes()
    dmin = 0.7
    while True:
        cases = build_cases(dmin)
        arrs, worst = {}, 0.0
        for tag in ZO.CASES:
            c = cases[tag]
            r64, mod = run_reference(ns, zbl_cls, agg_cls, c, torch.float64)
            r32, _ = run_reference(ns, zbl_cls, agg_cls, c, torch.float32)
            pre = tag + "_"
            for k in ("Z", "R", "cell", "offsets", "idx_i", "idx_j", "idx_m"):
                arrs[pre + k] = np.asarray(c[k])
            arrs[pre + "n_mol"] = np.asarray(c["n_mol"], dtype=np.int64)
            arrs[pre + "pbc"] = np.asarray(int(c["pbc"]), dtype=np.int64)
            arrs[pre + "rc"] = np.asarray(c["rc"], dtype=np.float64)
            arrs[pre + "energy_unit"], arrs[pre + "position_unit"] = np.asarray(c["energy_unit"]), np.asarray(c["position_unit"])
            arrs[pre + "energy_factor"] = np.asarray(project_units.convert_units("Ha", c["energy_unit"]))
            arrs[pre + "position_factor"] = np.asarray(project_units.convert_units("Bohr", c["position_unit"]))
            sd = mod.state_dict()
            for k in ("ke", "a_pow", "a_div", "exponents", "coefficients"):
                arrs[pre + k] = sd[k].detach().numpy().astype(np.float64)          # float32-rounded values, as both runs carried them
            arrs[pre + "state_keys"] = np.asarray(sorted(k for k in sd if not k.startswith("cutoff_fn")))
            for k in ("E", "E_atom", "F", "W", "agg"):
                arrs[pre + k], arrs[pre + k + "_f32"] = r64[k], r32[k]
                if k != "agg":
                    g = gap(r32[k], r64[k])
                    arrs[pre + "gap_" + k] = np.asarray(g)
                    worst = max(worst, g)
                    print("case %-6s %-6s float32 gap %.3e" % (tag, k, g))
        if worst < TOL / 4:
            break
        dmin += 0.1            # reshape the cases (never the tolerance): larger minimum distance
        print("gap %.3e >= %.3e: minimum distance raised to %.1f" % (worst, TOL / 4, dmin))
        assert dmin < 1.45
    arrs["min_distance"] = np.asarray(dmin)
    save_npz_reproducible(OUT, arrs)
    print("wrote %s: %d arrays, %d bytes, worst float32 gap %.3e, minimum distance %.1f" % (OUT, len(arrs), os.path.getsize(OUT), worst, dmin))


if __name__ == "__main__":
    main()
