"""Cost of the charge / spin embeddings in front of the fused force call, on the 256-frame aspirin batch, SchNet and PaiNN:

  (i)   the model with ``electronic_embeddings=[charge, spin]`` on the operator route (``spk_hip::electronic_embedding``, three launches each),
  (ii)  the same model object with the two embeddings forced onto their ATen route (``force_aten``: the reference's formula),
  (iii) the model without embeddings (the same interaction and head weights; the nuclear rows are looked up inside the first launch).

    python scripts/electronic_embedding_timing.py [rounds [calls per block [result.json]]]

Each is timed as HIP-graph replays (``GraphedForceCall``, what the MD loops run: device time) and as eager calls (host launch cost included), in
alternating blocks A B C A B C ... after a warm-up that also ramps the clock, with HIP events around each block of ``calls`` calls; the figure is
the median over the rounds of the per-call block time, the spread the inter-quartile range.  The operator alone is timed too, and the kernel
launches of one eager call are counted with the torch profiler (None where it is not available) and by the library's own tags.

The operator route is the default only if its median lies below the ATen median by more than both inter-quartile ranges together
(``hip_is_faster``)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from schnetpack_amd import _lib, model as M, nn as N, properties, synthetic as S
from schnetpack_amd.forcecall import GraphedForceCall

dev = torch.device("cuda:0")
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
TAGS = ("eembed_logit", "eembed_stats", "eembed_stack")


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


def embeddings():
    """[charge, spin] with every matrix of the stack non-zero (a fresh embedding's output layer is zero)."""
    torch.manual_seed(2)
    es = [N.ElectronicEmbedding(properties.total_charge, 128, is_charged=True), N.ElectronicEmbedding(properties.spin_multiplicity, 128, is_charged=False)]
    with torch.no_grad():
        for e in es:
            torch.nn.init.orthogonal_(e.resblock.linear.weight)
            for b in e.resblock.residual.stack:
                torch.nn.init.orthogonal_(b.linear2.weight)
            e.linear_q.bias.normal_()
    return es


def faster(t, a, b):
    """a below b by more than both inter-quartile ranges together"""
    return bool(t[b]["median_ms"] - t[a]["median_ms"] > t[a]["iqr_ms"] + t[b]["iqr_ms"])


def one_kind(kind, batch, inp):
    torch.manual_seed(0)
    plain = M.build_model(kind).to(dev).eval()
    with_e = M.build_model(kind, electronic_embeddings=embeddings())
    missing = with_e.representation.load_state_dict(plain.representation.state_dict(), strict=False)      # the same interactions and nuclear rows
    assert all(k.startswith("electronic_embeddings.") for k in missing.missing_keys) and not missing.unexpected_keys
    with_e.output_modules[0].load_state_dict(plain.output_modules[0].state_dict())
    with_e = with_e.to(dev).eval()
    embs = list(with_e.representation.electronic_embeddings)
    assert M.classify_potential(with_e) == 2 and M.classify_potential(plain) == 2 and all(e._act > 0 for e in embs)

    def route(aten):
        def call():
            for e in embs:
                e.force_aten = aten
            return with_e(dict(inp))
        return call

    calls = {"embed_hip": route(False), "embed_aten": route(True), "no_embedding": lambda: plain(dict(inp))}
    a, b = calls["embed_hip"](), calls["embed_aten"]()
    out = {"hip_vs_aten_rel": {k: float((a[k] - b[k]).abs().max() / b[k].abs().max()) for k in (properties.energy, properties.forces)}}
    for name, fn in calls.items():
        _lib.profile_enable(True)
        _lib.profile_report()
        fn()
        torch.cuda.synchronize()
        tags = _lib.profile_report()
        _lib.profile_enable(False)
        out["launches_" + name] = {"profiler_kernels": count_launches(fn), "tagged_total": int(sum(v[0] for v in tags.values())),
                                   "tagged_embedding": {k: v[0] for k, v in tags.items() if k in TAGS},
                                   "tagged_ms": {k: round(v[1], 5) for k, v in tags.items()}}
    out["eager"] = interleaved(calls)
    graphed = {}
    for name, aten in (("embed_hip", False), ("embed_aten", True), ("no_embedding", None)):
        try:
            for e in embs:
                e.force_aten = bool(aten)
            g = GraphedForceCall(plain if aten is None else with_e)
            g(inp)
            assert g.graph is not None
            graphed[name] = g.replay
        except Exception as exc:
            print("no graph for %s %s: %s" % (kind, name, exc), flush=True)
    for e in embs:
        e.force_aten = False
    if graphed:
        out["graph"] = interleaved(graphed)
    for key in ("eager", "graph"):
        if key in out and all(k in out[key] for k in calls):
            t = out[key]
            out[key + "_hip_minus_no_embedding_ms"] = round(t["embed_hip"]["median_ms"] - t["no_embedding"]["median_ms"], 5)
            out[key + "_aten_minus_no_embedding_ms"] = round(t["embed_aten"]["median_ms"] - t["no_embedding"]["median_ms"], 5)
            out[key + "_hip_is_faster"] = faster(t, "embed_hip", "embed_aten")
    # the operator alone (eager), against the module on ATen
    x = with_e.representation.embedding(inp[properties.Z]).detach()
    e0 = embs[0]
    ws = [w.detach() for w in e0.operator_weights()]
    psi, idx_m = inp[properties.total_charge], inp[properties.idx_m]

    def aten_alone():
        e0.force_aten = True
        with torch.no_grad():
            y = x + e0(x, inp)
        e0.force_aten = False
        return y

    out["operator"] = interleaved({"electronic_embedding": lambda: torch.ops.spk_hip.electronic_embedding(x, psi, idx_m, ws, True, e0._act, e0.epsilon, True),
                                   "aten_module": aten_alone})
    return out


def main():
    batch = S.molecule_batch("aspirin", 256, seed=0)
    inp = M.batch_to_inputs(batch, dev)
    n_mol = int(batch["n_mol"])
    rng = np.random.default_rng(1)
    inp[properties.total_charge] = torch.tensor(rng.integers(-2, 3, n_mol), dtype=torch.float32, device=dev)
    inp[properties.spin_multiplicity] = torch.tensor(rng.integers(0, 4, n_mol), dtype=torch.float32, device=dev)
    out = {"atoms": int(inp[properties.R].shape[0]), "n_mol": n_mol, "rounds": ROUNDS, "calls_per_block": CALLS}
    for kind in ("schnet", "painn"):
        out[kind] = one_kind(kind, batch, inp)
    print(json.dumps(out, indent=1), flush=True)
    if len(sys.argv) > 3:
        json.dump(out, open(sys.argv[3], "w"), indent=1)


if __name__ == "__main__":
    main()
