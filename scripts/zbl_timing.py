"""Cost of the ZBL term on the fused force call: the mode-4 call (standard potential + one ``zbl_forces`` launch) against the plain
standard-potential call (mode 2, code this feature does not touch) on the 256-frame aspirin batch and on the water box.

    python scripts/zbl_timing.py [rounds [calls per block [result.json]]]

Both models share one representation and one head.  The two calls are timed as HIP-graph replays (what the MD loops run) in alternating
blocks, A B A B ..., with HIP events around each block of ``calls`` replays; the figure is the median over the rounds of the per-call
block time, the spread the inter-quartile range.  For scale the ``zbl_forces`` operator alone (with and without the virial) and the existing
row passes over the same pairs -- ``pairwise_backward`` (``spk_pairwise_bwd_graph_f32``) and ``spk_edge_virial_f32`` (C ABI) -- are timed the same
way, as eager calls on the same stream."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from schnetpack_amd import _lib, model as M, ops, properties, synthetic as S
from schnetpack_amd._lib import fptr, iptr, stream
from schnetpack_amd.atomistic import Aggregation, Atomwise, Forces, PairwiseDistances, ZBLRepulsionEnergy
from schnetpack_amd.forcecall import GraphedForceCall
from schnetpack_amd.nn import CosineCutoff

dev = torch.device("cuda:0")
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 20


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


def measure(name, batch, kind):
    torch.manual_seed(0)
    plain = M.build_model(kind).to(dev).eval()
    rep, head = plain.representation, plain.output_modules[0]
    head2 = Atomwise(n_in=128, output_key="e_nn")
    head2.outnet = head.outnet
    zbl = M.NeuralNetworkPotential(rep, input_modules=[PairwiseDistances()],
                                   output_modules=[head2, ZBLRepulsionEnergy("eV", "Ang", "e_zbl", cutoff_fn=CosineCutoff(5.0)),
                                                   Aggregation(["e_nn", "e_zbl"], properties.energy), Forces()]).to(dev).eval()
    assert M.classify_potential(plain) == 2 and M.classify_potential(zbl) == 4
    inp = M.batch_to_inputs(batch, dev)
    calls = {"plain": GraphedForceCall(plain), "zbl": GraphedForceCall(zbl)}
    for c in calls.values():
        c(inp)
        assert c.graph is not None
    # the existing row passes over the same pairs: dE/dr -> atoms, dE/dr -> virial
    R, off, ii, jj, idx_m, n_mol = inp[properties.R], inp[properties.offsets], inp[properties.idx_i], inp[properties.idx_j], inp[properties.idx_m], int(batch["n_mol"])
    r = torch.ops.spk_hip.pairwise(R, ii, jj, off)
    prm = zbl.output_modules[1].op_params(R)
    gr = torch.ops.spk_hip.zbl_backward(torch.ones(n_mol, device=dev), r, inp[properties.Z], ii, jj, idx_m, n_mol, prm)
    F, W = torch.zeros_like(R), torch.zeros(n_mol, 3, 3, device=dev)
    L, plan = _lib.lib(), ops.EdgePlan(ii, jj, R.shape[0], r)
    vws = torch.empty(max(1, int(L.spk_edge_virial_workspace_bytes(plan.graph(), n_mol, 0))), dtype=torch.uint8, device=dev)
    Wv = torch.empty(n_mol, 3, 3, device=dev)

    def edge_virial():
        _lib.check(L.spk_edge_virial_f32(fptr(gr), fptr(R), fptr(off), plan.graph(), iptr(idx_m), n_mol, fptr(Wv), None, ctypes.c_void_p(vws.data_ptr()), stream()))
    fns = {"plain": calls["plain"].replay, "zbl": calls["zbl"].replay,
           "zbl_forces_launch": lambda: torch.ops.spk_hip.zbl_forces(R, off, inp[properties.Z], ii, jj, idx_m, n_mol, prm, F, None),
           "zbl_forces_virial_launch": lambda: torch.ops.spk_hip.zbl_forces(R, off, inp[properties.Z], ii, jj, idx_m, n_mol, prm, F, W),
           "pairwise_bwd": lambda: torch.ops.spk_hip.pairwise_backward(gr, ii, jj, R.shape[0]), "edge_virial": edge_virial}
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(block_ms(fn))
    res = {k: stats(v) for k, v in t.items()}
    res["difference_ms"] = round(res["zbl"]["median_ms"] - res["plain"]["median_ms"], 5)
    res["existing_pair_ms"] = round(res["pairwise_bwd"]["median_ms"] + res["edge_virial"]["median_ms"], 5)
    res.update(atoms=int(R.shape[0]), pairs=int(ii.shape[0]), kind=kind)
    print(name, kind, json.dumps(res), flush=True)
    return res


out = {}
for kind in ("schnet", "painn"):
    out["aspirin256_" + kind] = measure("aspirin x 256", S.molecule_batch("aspirin", 256, seed=0), kind)
    out["water_box_" + kind] = measure("water box", S.water_box(), kind)
if len(sys.argv) > 3:
    json.dump(out, open(sys.argv[3], "w"), indent=1)
