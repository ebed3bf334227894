"""Generator of tests/golden/tensorial_cases.npz (a plain script, not collected by pytest):

    python tests/make_tensorial_golden.py

It takes the reference's own ``GatedEquivariantBlock``, ``build_gated_equivariant_mlp`` (nn/equivariant.py, nn/blocks.py), ``DipoleMoment`` and
``Polarizability`` (atomistic/atomwise.py) at run time through oracle/refshim.py, runs them on seeded inputs -- the scalar and vector
"representations" are drawn, no representation network is needed -- and stores ONLY arrays: inputs, weights (float32 values), the float64
outputs, the reference's ``state_dict`` keys and shapes, and per quantity the reference's own float32 gap
``gap_* = max|x32 - x64| / max|x64|``.  The generator asserts every gap is below a quarter of the device tolerance (1e-5).

The gated weights of a case are shared by its ``DipoleMoment`` and ``Polarizability`` heads (one ``state_dict`` loaded into both: the two
classes build the same network), which keeps the fixture small.  Biases are drawn (the reference initialises them to zero, which would hide a
missing bias).  Positions lie within a few Angstrom of the origin so that the cancellation in sum q R stays inside the bar.  The reference
sizes its outputs by ``int(idx_m[-1]) + 1``; the trailing molecule without atoms of case b gets its expected zeros appended here.

Cases (each the smallest at which its path can go wrong):
  a   one 3-atom molecule, n_in = 64
  b   70 atoms in molecules of 1, 33, 0, 4, 32 atoms and a trailing empty one (n_mol = 6), n_in = 128: crosses a 32- and a 64-atom tile, ragged
      last tile, empty segments; dipole with / without total_charge and with correct_charges = False, charges, magnitude; the scalar
      ``DipoleMoment`` (build_mlp head) on the same inputs (arrays ``ds_*``)
  c   case b with one all-zero vector row (the norm has no epsilon)
  e   a head without a fused kernel: n_in = 64, n_layers = 3, n_hidden = 48
(case d, N = 0, needs no stored data: every output is empty or zero.)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim  # noqa: E402
from oracle.make_golden import save_npz_reproducible  # noqa: E402
import tensorial_oracle as TO  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tensorial_cases.npz")
TOL = 1.0e-5                 # the device parity contract; the reference's own float32 gap must stay below TOL / 4
SEED = 20251


def gap(x32, x64):
    scale = np.abs(x64).max()
    return float(np.abs(x32.astype(np.float64) - x64).max() / scale) if scale > 0 else float(np.abs(x32).max())


def geometry(tag, rng):
    if tag == "a":
        sizes, n_mol = [3], 1
    else:
        sizes, n_mol = [1, 33, 0, 4, 32, 0], 6
    idx_m = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    N = int(idx_m.shape[0])
    R = rng.uniform(-2.5, 2.5, (N, 3))
    total = np.asarray([1.0, -1.0, 0.0, 2.0, 0.0, 0.0][:n_mol])
    return idx_m, n_mol, np.asarray(sizes, dtype=np.int64), R, total


def draw_biases(net, gen):
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("bias"):
                p.copy_(0.2 * torch.randn(p.shape, generator=gen))


def state_layout(sd):
    keys = list(sd.keys())
    shapes = np.zeros((len(keys), 2), dtype=np.int64)
    for i, k in enumerate(keys):
        shapes[i, :sd[k].dim()] = list(sd[k].shape)
    return np.asarray(keys), shapes


def pad(x, n_mol):
    x = x.detach().numpy()
    return np.concatenate([x, np.zeros((n_mol - x.shape[0],) + x.shape[1:], dtype=x.dtype)])


def run_reference(ns, heads, c, dtype):
    """Every stored output of one case from the reference's own modules in ``dtype``."""
    P = ns.properties
    maxm = int(c["idx_m"][-1]) + 1
    n_mol = int(c["n_mol"])

    def inputs(with_q):
        inp = {P.R: torch.tensor(c["R"], dtype=dtype), "scalar_representation": torch.tensor(c["s"], dtype=dtype),
               "vector_representation": torch.tensor(c["v"], dtype=dtype), P.idx_m: torch.tensor(c["idx_m"]),
               P.n_atoms: torch.tensor(c["n_atoms"][:maxm])}
        if with_q:
            inp[P.total_charge] = torch.tensor(c["total_charge"][:maxm], dtype=dtype)
        return inp

    out = {}
    with torch.no_grad():
        dv = heads["dv_plain"].to(dtype)
        s_out, v_out = dv.outnet((torch.tensor(c["s"], dtype=dtype), torch.tensor(c["v"], dtype=dtype)))
        out["gm_s"], out["gm_v"] = s_out.numpy(), v_out.numpy()
        for name, (correct, with_q) in TO.VARIANTS.items():
            res = heads["dv_" + name].to(dtype)(inputs(with_q))
            out["mu_" + name], out["charges_" + name] = pad(res[P.dipole_moment], n_mol), res[P.partial_charges].numpy()
        out["mag_plain"] = pad(heads["dv_mag"].to(dtype)(inputs(False))[P.dipole_moment], n_mol)
        out["alpha"] = pad(heads["pol"].to(dtype)(inputs(False))[P.polarizability], n_mol)
        if "ds_plain" in heads:
            out["ds_q"] = heads["ds_plain"].to(dtype).outnet(torch.tensor(c["s"], dtype=dtype)).numpy()
            for name, (correct, with_q) in TO.VARIANTS.items():
                res = heads["ds_" + name].to(dtype)(inputs(with_q))
                out["ds_mu_" + name], out["ds_charges_" + name] = pad(res[P.dipole_moment], n_mol), res[P.partial_charges].numpy()
    return out


def build_heads(ns, n_in, n_layers, n_hidden, gen, scalar):
    A = ns.atomwise
    kw = dict(n_in=n_in, n_hidden=n_hidden if n_hidden else None, n_layers=n_layers)
    torch.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=gen)))
    heads = {}
    for name, (correct, _) in TO.VARIANTS.items():
        heads["dv_" + name] = A.DipoleMoment(use_vector_representation=True, return_charges=True, correct_charges=correct, **kw)
    heads["dv_mag"] = A.DipoleMoment(use_vector_representation=True, predict_magnitude=True, **kw)
    heads["pol"] = A.Polarizability(**kw)
    draw_biases(heads["dv_plain"].outnet, gen)
    for k, h in heads.items():
        if k != "dv_plain":
            h.outnet.load_state_dict(heads["dv_plain"].outnet.state_dict())
    if scalar:
        for name, (correct, _) in TO.VARIANTS.items():
            heads["ds_" + name] = A.DipoleMoment(use_vector_representation=False, return_charges=True, correct_charges=correct, n_in=n_in)
        draw_biases(heads["ds_plain"].outnet, gen)
        for name in TO.VARIANTS:
            heads["ds_" + name].outnet.load_state_dict(heads["ds_plain"].outnet.state_dict())
    return heads


def main():
    ns = refshim.load()
    assert ns.nn.GatedEquivariantBlock is not None and ns.nn.build_gated_equivariant_mlp is not None
    rng = np.random.default_rng(SEED)
    gen = torch.Generator().manual_seed(SEED)
    arrs, worst = {}, 0.0
    shared = {}
    for tag, (n_in, n_layers, n_hidden) in TO.CASES.items():
        pre = tag + "_"
        if tag == "c":                                   # case b with one all-zero vector row
            c, heads = dict(shared["c"]), shared["heads"]
            c["v"] = c["v"].copy()
            c["v"][40] = 0.0
        else:
            idx_m, n_mol, n_atoms, R, total = geometry(tag, rng)
            N = idx_m.shape[0]
            # float32-representable inputs: both runs and the device see the same numbers
            c = dict(idx_m=idx_m, n_mol=np.asarray(n_mol, dtype=np.int64), n_atoms=n_atoms, R=R.astype(np.float32).astype(np.float64),
                     total_charge=total, s=(0.7 * rng.standard_normal((N, n_in))).astype(np.float32).astype(np.float64),
                     v=(0.7 * rng.standard_normal((N, 3, n_in))).astype(np.float32).astype(np.float64))
            heads = build_heads(ns, n_in, n_layers, n_hidden, gen, scalar=tag == "b")
            if tag == "b":
                shared["c"], shared["heads"] = c, heads
        for h in heads.values():
            h.float()
        gm_sd = heads["dv_plain"].state_dict()
        for k in ("idx_m", "n_mol", "n_atoms", "R", "total_charge", "s", "v"):
            arrs[pre + k] = c[k].astype(np.float32) if k in ("s", "v") else c[k]          # (float32 values: stored as such)
        if tag != "c":                                   # (case c reads the weights of case b)
            for i, (k, w) in enumerate(gm_sd.items()):
                arrs[pre + "gm_w%d" % i] = w.detach().numpy().astype(np.float32)
            arrs[pre + "dv_state_keys"], arrs[pre + "dv_state_shapes"] = state_layout(gm_sd)
            arrs[pre + "pol_state_keys"], arrs[pre + "pol_state_shapes"] = state_layout(heads["pol"].state_dict())
            if "ds_plain" in heads:
                ds_sd = heads["ds_plain"].state_dict()
                for i, (k, w) in enumerate(ds_sd.items()):
                    arrs[pre + "ds_w%d" % i] = w.detach().numpy().astype(np.float32)
                arrs[pre + "ds_state_keys"], arrs[pre + "ds_state_shapes"] = state_layout(ds_sd)
        r32 = run_reference(ns, heads, c, torch.float32)
        r64 = run_reference(ns, heads, c, torch.float64)
        for k in r64:
            arrs[pre + k] = r64[k]
            g = gap(r32[k], r64[k])
            arrs[pre + "gap_" + k] = np.asarray(g)
            worst = max(worst, g)
            print("case %s %-18s float32 gap %.3e" % (tag, k, g))
            assert g < TOL / 4, "the reference's own float32 gap of %s / %s is not below a quarter of the tolerance: reshape the case" % (tag, k)
    save_npz_reproducible(OUT, arrs)
    print("wrote %s: %d arrays, %d bytes, worst float32 gap %.3e" % (OUT, len(arrs), os.path.getsize(OUT), worst))


if __name__ == "__main__":
    main()
