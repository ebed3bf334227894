"""Force calls of SO3net potentials: the HIP route of the SO(3) layers (``real_sph_harm``, ``so3_conv``, ``so3_product``) against the mirrors' own ATen
route -- the reference's formula on the same device and tensors, what a user who loads an SO3net model gets without these kernels.

    python scripts/so3net_timing.py [rounds [calls per block [result.json]]]

  (i)   the reference's trained Si16 potential (weights: tests/golden/so3_cases.npz; n_atom_basis 64, 2 interactions, lmax 2, cutoff 7), energy +
        forces + stress, on the jittered 16-atom cell and on its 3 x 3 x 3 replica (432 atoms)
  (ii)  SO3net(64, 2, lmax = 2, GaussianRBF(20, 5.0)) + Atomwise + Forces on the 256-frame aspirin batch; peak extra memory of one call, both routes
  (iii) (ii) at lmax = 1 and 3
Both routes run the same model object: the ATen route is selected by putting the three SO(3) layer kinds (and nothing else) into training mode,
which is what their route switch reads.  One process; 5 warm-up calls each; the routes are timed in alternating blocks of ``calls`` calls between
HIP events; the figure is the median over the rounds of the per-call block time, the spread the inter-quartile range."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from schnetpack_amd import atomistic as A, model as M, synthetic as S
from schnetpack_amd.nn import CosineCutoff, GaussianRBF, so3
from schnetpack_amd.representation import SO3net

dev = torch.device("cuda:0")
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
SO3_LAYERS = (so3.RealSphericalHarmonics, so3.SO3Convolution, so3.SO3TensorProduct)


def block_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / CALLS


def stats(xs):
    q = np.percentile(np.asarray(xs), [25, 50, 75])
    return {"median_ms": round(float(q[1]), 5), "iqr_ms": round(float(q[2] - q[0]), 5)}


def peak_extra_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)


def route(model, hip):
    for m in model.modules():
        if isinstance(m, SO3_LAYERS):
            m.train(not hip)


def force_call(model, inputs, hip):
    def call():
        route(model, hip)
        return model(dict(inputs))
    return call


def compare(name, model, inputs, keys, extra=None, memory=False):
    fns = {"hip": force_call(model, inputs, True), "aten": force_call(model, inputs, False)}
    outs = {k: fn() for k, fn in fns.items()}
    agree = {k: float((outs["hip"][k] - outs["aten"][k]).abs().max() / outs["aten"][k].abs().max()) for k in keys}
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(block_ms(fn))
    res = {k: stats(v) for k, v in t.items()}
    res["speedup"] = round(res["aten"]["median_ms"] / res["hip"]["median_ms"], 2)
    res["hip_below_aten_by_more_than_both_iqr"] = bool(res["aten"]["median_ms"] - res["hip"]["median_ms"] > res["aten"]["iqr_ms"] + res["hip"]["iqr_ms"])
    res["routes_agree"] = agree
    if memory:
        res.update(peak_extra_mib_hip=peak_extra_mib(fns["hip"]), peak_extra_mib_aten=peak_extra_mib(fns["aten"]))
    res.update(extra or {})
    print(name, json.dumps(res), flush=True)
    return res


def all_images_list(R, cell, cutoff):
    """Directed pairs (i, j, image) within the cutoff, sorted by i, then j, then image (numpy float64; symmetric by construction)."""
    nmax = np.ceil(cutoff * np.linalg.norm(np.linalg.inv(cell), axis=0)).astype(int)
    sh = np.asarray([(a, b, c) for a in range(-nmax[0], nmax[0] + 1) for b in range(-nmax[1], nmax[1] + 1) for c in range(-nmax[2], nmax[2] + 1)], dtype=np.float64)
    off = sh @ cell
    ii, jj, oo = [], [], []
    for i in range(R.shape[0]):                                                   # row by row: the replica has 432 x 432 x 27 candidates
        d = np.linalg.norm(R[None, :, :] - R[i] + off[:, None, :], axis=-1)      # [images, atoms]
        k, j = np.nonzero((d < cutoff) & (d > 0.0))
        order = np.lexsort((k, j))
        ii.append(np.full(len(j), i)), jj.append(j[order]), oo.append(off[k[order]])
    return np.concatenate(ii), np.concatenate(jj), np.concatenate(oo)


def cell_inputs(R, cell, cutoff):
    ii, jj, off = all_images_list(R, cell, cutoff)
    n = R.shape[0]
    f = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    return {"_atomic_numbers": torch.full((n,), 14, device=dev), "_positions": f(R), "_cell": f(cell[None]), "_offsets": f(off),
            "_idx_i": torch.tensor(ii, device=dev), "_idx_j": torch.tensor(jj, device=dev), "_idx_m": torch.zeros(n, dtype=torch.long, device=dev),
            "_n_atoms": torch.tensor([n], device=dev), "_pbc": torch.ones(1, 3, dtype=torch.bool, device=dev), "_n_molecules": 1}


out = {}
# (i) the trained Si16 potential
G = np.load(os.path.join(ROOT, "tests", "golden", "so3_cases.npz"))
si = M.NeuralNetworkPotential(SO3net(64, 2, 2, GaussianRBF(20, 7.0), CosineCutoff(7.0)), input_modules=[A.Strain(), A.PairwiseDistances()],
                              output_modules=[A.Atomwise(64, output_key="energy"), A.Forces(calc_stress=True)])
si.load_state_dict({str(name): torch.tensor(G["m1_w%d" % k]) for k, name in enumerate(G["m1_wkeys"])}, strict=True)
si = si.to(dev).eval()
R, cell = G["m1_R"], G["m1_cell"][0]
shifts = np.asarray([(a, b, c) for a in range(3) for b in range(3) for c in range(3)], dtype=np.float64) @ cell
for name, (Rk, ck) in {"si16": (R, cell), "si432": ((R[None] + shifts[:, None]).reshape(-1, 3), 3.0 * cell)}.items():
    inp = cell_inputs(Rk, ck, 7.0)
    out[name] = compare("(i) Si potential, %s" % name, si, inp, ("energy", "forces", "stress"),
                        dict(atoms=int(Rk.shape[0]), pairs=int(inp["_idx_i"].shape[0])))

# (ii), (iii) the aspirin batch
asp = M.batch_to_inputs(S.molecule_batch("aspirin", 256, seed=0), dev)
for lmax in (2, 1, 3):
    torch.manual_seed(0)
    model = M.NeuralNetworkPotential(SO3net(64, 2, lmax, GaussianRBF(20, 5.0), CosineCutoff(5.0)), input_modules=[A.PairwiseDistances()],
                                     output_modules=[A.Atomwise(64, output_key="energy"), A.Forces()]).to(dev).eval()
    out["aspirin256_lmax%d" % lmax] = compare("(ii/iii) aspirin x 256, lmax %d" % lmax, model, asp, ("energy", "forces"),
                                              dict(atoms=int(asp["_atomic_numbers"].shape[0]), pairs=int(asp["_idx_i"].shape[0])), memory=lmax == 2)
if len(sys.argv) > 3:
    json.dump(out, open(sys.argv[3], "w"), indent=1)
