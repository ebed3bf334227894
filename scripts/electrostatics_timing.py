"""Forward + backward (E, dE/dR or dE/dr_ij, dE/dq) of the electrostatic terms: the HIP operators against the module mirrors' own ATen route
(the reference's formula on the same device and tensors -- what a user gets by running the reference's module on GPU tensors).

    python scripts/electrostatics_timing.py [rounds [calls per block [result.json]]]

  (i)   ``ewald_recip`` on the 31 944-atom water box, charges -0.8476 / +0.4238 by element, k_max = 4 (K = 340); peak extra memory of one
        forward + backward on both routes
  (ii)  ``EnergyCoulomb`` (damped, shifted cutoff 4.5 on the 5 A list) on the 256-frame aspirin batch
  (iii) the real-space Ewald term on the water box with its existing 5 A list
One process; 5 warm-up calls each; the routes are timed in alternating blocks of ``calls`` calls between HIP events; the figure is the median
over the rounds of the per-call block time, the spread the inter-quartile range.  The forward of (i) alone is timed as well: its structure-factor
kernel does about 8 flops per (atom, k)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from schnetpack_amd import atomistic as A, model as M, properties, synthetic as S
from schnetpack_amd.nn import SwitchFunction

dev = torch.device("cuda:0")
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10


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


def compare(name, fns, extra=None):
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
    res.update(extra or {})
    print(name, json.dumps(res), flush=True)
    return res


def pair_inputs(batch):
    inp = M.batch_to_inputs(batch, dev)
    with torch.no_grad():
        r = torch.ops.spk_hip.pairwise(inp[properties.R], inp[properties.idx_i], inp[properties.idx_j], inp[properties.offsets])
    inp[properties.Rij] = r.requires_grad_()
    return inp


def pair_call(mod, inp, q):
    def call():
        E = mod(dict(inp, **{properties.partial_charges: q}))["e"]
        return torch.autograd.grad(E.sum(), [inp[properties.Rij], q])
    return call


out = {}
water = S.water_box()
q_w = torch.where(water["Z"] == 8, torch.tensor(-0.8476), torch.tensor(0.4238)).to(dev).requires_grad_()
inp_w = pair_inputs(water)
inp_w[properties.cell] = water["cell"].float()[None].to(dev)
R_w = inp_w[properties.R].requires_grad_()
N, n_pairs_w = int(R_w.shape[0]), int(inp_w[properties.idx_i].shape[0])

# (i) the reciprocal-space sum
ew = A.EnergyEwald(0.16, 4, "eV", "Ang", "e", use_neighbors_lr=False).to(dev).eval()
prm = ew.op_params(R_w)
K = int(ew.kvecs.shape[0])


def recip_hip():
    E = torch.ops.spk_hip.ewald_recip(R_w, q_w, inp_w[properties.cell], inp_w[properties.idx_m], 1, ew.kvecs, prm[8:10])[0]
    return torch.autograd.grad(E.sum(), [R_w, q_w])


def recip_aten():
    E = ew._reciprocal_space(q_w, R_w, inp_w[properties.cell], inp_w[properties.idx_m], 1)
    return torch.autograd.grad(E.sum(), [R_w, q_w])


def recip_fwd():
    with torch.no_grad():
        return torch.ops.spk_hip.ewald_recip(R_w, q_w, inp_w[properties.cell], inp_w[properties.idx_m], 1, ew.kvecs, prm[8:10])[0]


a, b = recip_hip(), recip_aten()
agree = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(a, b)]
mem = {"peak_extra_mib_hip": peak_extra_mib(recip_hip), "peak_extra_mib_aten": peak_extra_mib(recip_aten)}
out["ewald_recip_water"] = compare("(i) ewald_recip, water box", {"hip": recip_hip, "aten": recip_aten, "hip_forward_only": recip_fwd},
                                   dict(mem, atoms=N, kvecs=K, routes_agree_gR_gq=agree))
fwd_ms = out["ewald_recip_water"]["hip_forward_only"]["median_ms"]
out["ewald_recip_water"]["forward_gflops_at_8_per_atom_k"] = round(8.0 * N * K / (fwd_ms * 1e-3) / 1e9, 1)

# (ii) damped, shifted Coulomb on the aspirin batch
asp = S.molecule_batch("aspirin", 256, seed=0)
inp_a = pair_inputs(asp)
q_a = (0.4 * torch.randn(inp_a[properties.R].shape[0], generator=torch.Generator().manual_seed(0))).to(dev).requires_grad_()
mk = lambda: A.EnergyCoulomb("eV", "Ang", A.DampedCoulombPotential(SwitchFunction(1.0, 3.0)), "e", use_neighbors_lr=False, cutoff=4.5).to(dev)
out["coulomb_aspirin256"] = compare("(ii) EnergyCoulomb, aspirin x 256", {"hip": pair_call(mk().eval(), inp_a, q_a), "aten": pair_call(mk().train(), inp_a, q_a)},
                                    dict(atoms=int(q_a.shape[0]), pairs=int(inp_a[properties.idx_i].shape[0])))

# (iii) the real-space Ewald term on the water box


def real_call(train):
    mod = A.EnergyEwald(0.16, 4, "eV", "Ang", "e", use_neighbors_lr=False).to(dev)
    if train:
        def call():
            d = inp_w[properties.Rij].norm(dim=1)
            E = mod._real_space(q_w, d, inp_w[properties.idx_i], inp_w[properties.idx_j], inp_w[properties.idx_m], N, 1)
            return torch.autograd.grad(E.sum(), [inp_w[properties.Rij], q_w])
        return call
    p8 = mod.op_params(R_w)[0:8]

    def call():
        E = torch.ops.spk_hip.coulomb(inp_w[properties.Rij], q_w, inp_w[properties.idx_i], inp_w[properties.idx_j], inp_w[properties.idx_m], 1, p8)[0]
        return torch.autograd.grad(E.sum(), [inp_w[properties.Rij], q_w])
    return call


out["ewald_real_water"] = compare("(iii) Ewald real space, water box", {"hip": real_call(False), "aten": real_call(True)}, dict(atoms=N, pairs=n_pairs_w))
if len(sys.argv) > 3:
    json.dump(out, open(sys.argv[3], "w"), indent=1)
