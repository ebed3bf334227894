"""Cost of the tensorial heads behind the fused force call, on the 256-frame aspirin PaiNN batch:

  (i)   the mode-2 force call alone (code this feature does not touch),
  (ii)  the same call with ``DipoleMoment(use_vector_representation=True)`` + ``Polarizability`` on the new operators,
  (iii) the same model with the two heads forced onto their ATen route (the reference's formula on the ``Dense`` / ``scatter_add`` mirrors).

    python scripts/tensorial_timing.py [rounds [calls per block [result.json]]]

The three models share one representation and one energy head; (ii) and (iii) share the head weights too.  Each is timed twice: as HIP-graph
replays (``GraphedForceCall``, what the MD loops run: device time) and as eager calls (host launch cost included), in alternating blocks
A B C A B C ... after a warm-up that also ramps the clock, with HIP events around each block of ``calls`` calls; the figure is the median over
the rounds of the per-call block time, the spread the inter-quartile range.  The two new operators of a head are also timed alone, and the
kernel launches of one eager call of each model are counted with the torch profiler (None where it is not available)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from schnetpack_amd import _lib, model as M, properties, synthetic as S
from schnetpack_amd.atomistic import DipoleMoment, Forces, PairwiseDistances, Polarizability
from schnetpack_amd.forcecall import GraphedForceCall

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


def interleaved(fns):
    for fn in fns.values():            # warm-up of every shape, and the clock ramp
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(block_ms(fn))
    return {k: stats(v) for k, v in t.items()}


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n if n > 0 else None
    except Exception as exc:           # no tracer in this build
        print("launch count unavailable:", exc, flush=True)
        return None


def heads(fused):
    torch.manual_seed(1)
    hs = [DipoleMoment(n_in=128, use_vector_representation=True), Polarizability(n_in=128)]
    if not fused:
        for h in hs:
            assert h._gated_act > 0
            h._gated_act = 0           # no kernel for this head: the reference's formula on the mirrors
    return hs


def main():
    batch = S.molecule_batch("aspirin", 256, seed=0)
    torch.manual_seed(0)
    plain = M.build_model("painn").to(dev).eval()
    rep, head = plain.representation, plain.output_modules[0]
    mk = lambda fused: M.NeuralNetworkPotential(rep, input_modules=[PairwiseDistances()], output_modules=[head, Forces()] + heads(fused)).to(dev).eval()
    models = {"force_call": plain, "heads_hip": mk(True), "heads_aten": mk(False)}
    assert all(M.classify_potential(m) == 2 for m in models.values())
    inp = M.batch_to_inputs(batch, dev)
    with torch.no_grad():
        a, b = models["heads_hip"](dict(inp)), models["heads_aten"](dict(inp))
    err = {k: float((a[k] - b[k]).abs().max() / b[k].abs().max()) for k in (properties.dipole_moment, properties.polarizability)}
    assert torch.equal(a[properties.forces], b[properties.forces])
    out = {"atoms": int(inp[properties.R].shape[0]), "n_mol": int(batch["n_mol"]), "hip_vs_aten_rel": err}
    # launches of one eager call: the library's own tags (its kernels only) and the profiler's count (every kernel)
    for name, m in models.items():
        _lib.profile_enable(True)
        _lib.profile_report()
        with torch.no_grad():
            m(dict(inp))
        torch.cuda.synchronize()
        tags = _lib.profile_report()
        _lib.profile_enable(False)
        out["launches_" + name] = {"profiler_kernels": count_launches(lambda m=m: m(dict(inp))),
                                   "tagged": {k: v[0] for k, v in tags.items() if k in ("gated_mlp", "moment_reduce")}}
    eager = {name: (lambda m=m: m(dict(inp))) for name, m in models.items()}
    out["eager"] = interleaved(eager)
    graphed = {}
    for name, m in models.items():
        try:
            g = GraphedForceCall(m)
            g(inp)
            assert g.graph is not None
            graphed[name] = g.replay
        except Exception as exc:
            print("no graph for %s: %s" % (name, exc), flush=True)
    if graphed:
        out["graph"] = interleaved(graphed)
    # the two operators of one head alone (eager)
    with torch.no_grad():
        fused = models["heads_hip"]._potential_forces_forward(dict(inp))
    x, mu, R, idx_m, n_mol = fused["scalar_representation"], fused["vector_representation"], inp[properties.R], inp[properties.idx_m], int(batch["n_mol"])
    ws = models["heads_hip"].output_modules[2]._head_weights()
    q, d = torch.ops.spk_hip.gated_mlp(x, mu, ws, _lib.SPK_ACT_SILU)
    out["operators"] = interleaved({"gated_mlp": lambda: torch.ops.spk_hip.gated_mlp(x, mu, ws, _lib.SPK_ACT_SILU),
                                    "dipole_moment": lambda: torch.ops.spk_hip.dipole_moment(q, d, R, idx_m, n_mol, None, True),
                                    "polarizability": lambda: torch.ops.spk_hip.polarizability(q, d, R, idx_m, n_mol)})
    for key in ("eager", "graph"):
        if key in out and all(k in out[key] for k in models):
            t = out[key]
            out[key + "_heads_hip_minus_call_ms"] = round(t["heads_hip"]["median_ms"] - t["force_call"]["median_ms"], 5)
            out[key + "_heads_aten_minus_call_ms"] = round(t["heads_aten"]["median_ms"] - t["force_call"]["median_ms"], 5)
    print(json.dumps(out, indent=1), flush=True)
    if len(sys.argv) > 3:
        json.dump(out, open(sys.argv[3], "w"), indent=1)


if __name__ == "__main__":
    main()
