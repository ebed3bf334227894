"""Generator of tests/golden/embedding_cases.npz (a plain script, not collected by pytest):

    python tests/make_embedding_golden.py

It runs the reference's own ``nn.ElectronicEmbedding`` / ``nn.NuclearEmbedding`` and its ``SchNet`` / ``PaiNN`` potentials (through oracle/refshim.py)
on the CPU and stores ONLY arrays.  Inputs and weights are the float32 roundings of the seeded streams of tests/embedding_oracle.py and are NOT
stored (the 256-wide case and the 128-wide models would not fit a committed file); their checksum is.

  sd_<ee|ne|res|stack|mlp>_keys / _shapes  ``state_dict`` keys and shapes of ElectronicEmbedding("total_charge", 64, True, 2), NuclearEmbedding(101, 64),
                                           Residual(64, ssp), ResidualStack(64, 2, ssp) and ResidualMLP(64, 1, ssp)
  ne_table                                 the eval table of a seeded NuclearEmbedding(101, 64, zero_init=False), float64
  <case>_out / _gap / _checksum            per operator case of ``embedding_oracle.CASES``: the embedding from a float64 run (every row; the two
                                           4 500-atom cases: ``PAIR_ROWS`` and, as ``_alpha``, the attention weight of every atom), the reference's
                                           own float32 run against float64 (max-norm relative), the checksum of inputs and weights
  m<k>_energy / _forces / _scalar_representation / _gap_* / _checksum / _sd_keys / _sd_shapes     the model cases (the representation on
                                           ``embedding_oracle.rep_rows``)
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
import embedding_oracle as EO  # noqa: E402
from make_so3_golden import sd_arrays  # noqa: E402

GAP_BOUND = 5.0e-6


def reference():
    ns = refshim.load()
    if not hasattr(sys.modules["ase.data"], "atomic_masses"):
        sys.modules["ase.data"].atomic_masses = np.ones(119)
    return ns


def activation(ns, name):
    return ns.nn.shifted_softplus if name == "ssp" else torch.nn.functional.silu


def operator_case(ns, name, out):
    c = EO.case(name)
    emb = ns.nn.ElectronicEmbedding("psi", c["F"], c["charged"], num_residual=c["n_res"], activation=activation(ns, c["act"]), epsilon=EO.EPS)
    names = [k for k, _ in emb.named_parameters()]
    assert len(names) == len(c["ws"]), names
    with torch.no_grad():
        for (k, p), w in zip(emb.named_parameters(), c["ws"]):      # the reference's parameter order IS the operator's weight order
            assert tuple(p.shape) == w.shape, (k, p.shape, w.shape)
            p.copy_(torch.tensor(w))
    n_mol = len(c["psi"])

    def run(dtype):
        m = emb.to(dtype).eval()
        inp = {"_idx": torch.arange(n_mol), "_idx_m": torch.tensor(c["idx_m"]), "psi": torch.tensor(c["psi"], dtype=dtype)}
        with torch.no_grad():
            return m(torch.tensor(c["x"], dtype=dtype), inp).double().numpy()

    y64 = run(torch.float64)
    emb.float()
    y32 = run(torch.float32)
    gap = float(np.abs(y32 - y64).max() / np.abs(y64).max())
    mine, alpha = EO.embedding(c["x"], c["psi"], c["idx_m"], c["ws"], c["charged"], c["act"], return_alpha=True)
    print("%-12s N %5d  float32 gap %.2e   oracle %.1e   without the eps term %.1e" % (
        name, len(c["idx_m"]), gap, EO.rel(mine, y64), EO.rel(EO.embedding(c["x"], c["psi"], c["idx_m"], c["ws"], c["charged"], c["act"], eps_term=False), y64)))
    assert name == "silu" or gap <= GAP_BOUND, (name, gap)
    rows = EO.PAIR_ROWS if name.startswith("pairs") else np.arange(len(y64))
    out[name + "_out"] = y64[rows]
    if name.startswith("pairs"):
        out[name + "_alpha"] = alpha
    out[name + "_gap"] = np.asarray(gap)
    out[name + "_checksum"] = np.asarray(EO.checksum([c["x"], c["psi"]] + c["ws"]))


def spk_namespace(ns):
    """The reference's classes under the names ``embedding_oracle.build_model`` asks for."""
    import types
    rep = types.SimpleNamespace(SchNet=ns.schnet.SchNet, PaiNN=ns.painn.PaiNN)
    atom = types.SimpleNamespace(PairwiseDistances=ns.distances.PairwiseDistances, Atomwise=ns.atomwise.Atomwise, Forces=ns.response.Forces)
    return types.SimpleNamespace(atomistic=atom, nn=ns.nn, representation=rep, model=ns.model)


def run_model(model, arrs, dtype, keys):
    m = model.to(dtype).eval()
    inp = EO.model_inputs(arrs, dtype, "cpu")
    inp.pop("_n_molecules")
    inp = m.initialize_derivatives(inp)
    for mod in m.input_modules:
        inp = mod(inp)
    inp = m.representation(inp)
    for mod in m.output_modules:
        inp = mod(inp)
    return {k: inp[k].detach().double().numpy() for k in keys}


def model_case(ns, tag, out):
    arrs = EO.model_arrays(tag)
    model = EO.build_model(tag, spk_namespace(ns))
    keys = EO.MODEL_KEYS[tag]
    r64 = run_model(model, arrs, torch.float64, keys)
    model.float()
    r32 = run_model(model, arrs, torch.float32, keys)
    sd_arrays(tag + "_sd", model.state_dict(), out)
    params = EO.seeded_parameters(EO.parameter_shapes(model), EO.MODEL_WEIGHTS[tag])
    out[tag + "_checksum"] = np.asarray(EO.checksum([arrs[k] for k in sorted(arrs)] + [params[k] for k in sorted(params)]))
    rows = EO.rep_rows(tag, len(arrs["Z"]))
    for k in keys:
        gap = float(np.abs(r32[k] - r64[k]).max() / np.abs(r64[k]).max())
        out["%s_gap_%s" % (tag, k)] = np.asarray(gap)
        out["%s_%s" % (tag, k)] = r64[k][rows] if k == "scalar_representation" else r64[k]
        print("%s %-24s float32 gap %.2e   |max| %.3g" % (tag, k, gap, np.abs(r64[k]).max()))
        assert gap <= GAP_BOUND, (tag, k, gap)


def main():
    torch.set_num_threads(1)      # one summation order: the float32 gaps, too, regenerate byte for byte
    torch.use_deterministic_algorithms(True)
    ns = reference()
    out = {}
    ssp = ns.nn.shifted_softplus
    blocks = sys.modules["schnetpack.nn.blocks"]
    sd_arrays("sd_ee", ns.nn.ElectronicEmbedding("total_charge", 64, True, num_residual=2).state_dict(), out)
    sd_arrays("sd_ne", ns.nn.NuclearEmbedding(101, 64).state_dict(), out)
    sd_arrays("sd_res", blocks.Residual(64, ssp).state_dict(), out)
    sd_arrays("sd_stack", blocks.ResidualStack(64, 2, ssp).state_dict(), out)
    sd_arrays("sd_mlp", blocks.ResidualMLP(64, 1, ssp).state_dict(), out)
    ne = EO.load_seeded(ns.nn.NuclearEmbedding(101, 64, zero_init=False), "ne").double()
    ne.eval()
    out["ne_table"] = ne.embedding.detach().numpy().copy()
    out["ne_checksum"] = np.asarray(EO.checksum(list(EO.seeded_parameters(EO.parameter_shapes(ne), "ne").values())))
    for name in EO.CASES:
        operator_case(ns, name, out)
    for tag in ("m1", "m2", "m3", "m4"):
        model_case(ns, tag, out)
    save_npz_reproducible(EO.GOLDEN, out)
    print("wrote %s: %d arrays, %d bytes" % (EO.GOLDEN, len(out), os.path.getsize(EO.GOLDEN)))


if __name__ == "__main__":
    main()
