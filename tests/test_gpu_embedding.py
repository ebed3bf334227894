"""GPU: the electronic embedding (csrc/spk_eembed.hip) through every route -- the C ABI, ``torch.ops.spk_hip.electronic_embedding`` (both
``add_input`` values) and the ``nn.ElectronicEmbedding`` mirror -- against the fixture of the reference's own classes
(tests/golden/embedding_cases.npz) and the float64 oracle pinned to it (tests/embedding_oracle.py, tests/test_embedding_reference.py), and the
models m1 - m4 through ``NeuralNetworkPotential``.

Bounds.  On ``x + out`` -- what the model consumes -- the project's parity bar, 1e-5 max-norm relative.  On ``out`` alone per case
``max(1e-5, 2 gap_case)``, gap_case being the reference's own float32 run against float64 (stored by the generator): two independent float32
evaluations of the same formula may each be that far from it.  Every test prints what it measured.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import embedding_oracle as EO  # noqa: E402

from schnetpack_amd import _lib, model as M, nn as N, properties  # noqa: E402
from schnetpack_amd._lib import fptr, iptr, stream  # noqa: E402
from schnetpack_amd.nn.fallback import fallback_count  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1.0e-5
G = EO.gold()
ACTS = {"ssp": N.shifted_softplus, "silu": torch.nn.functional.silu, "tanh": torch.tanh}
TAGS = {"eembed_logit", "eembed_stats", "eembed_stack"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    return torch.device("cuda", 0)


_CASES = {}


def case(name, dev):
    """An operator case on the device (built once, never modified): arrays, device tensors, the float64 oracle, the bound on ``out``."""
    if name not in _CASES:
        c = EO.check_streams(G, name)
        c["xd"] = torch.tensor(c["x"], device=dev)
        c["psid"] = torch.tensor(c["psi"], device=dev)
        c["idxd"] = torch.tensor(c["idx_m"], device=dev)
        c["wd"] = [torch.tensor(w, device=dev) for w in c["ws"]]
        c["oracle"] = EO.embedding(c["x"], c["psi"], c["idx_m"], c["ws"], c["charged"], c["act"])
        c["want"], c["rows"] = EO.expected(G, name)
        assert EO.rel(c["oracle"][c["rows"]], c["want"]) < 1e-12
        c["bound"] = max(TOL, 2.0 * float(G[name + "_gap"]))
        _CASES[name] = c
    return _CASES[name]


def c_embed(x, psi, idx_m, ws, charged, act_id, add_input=False, eps=EO.EPS, n_mol=None):
    N_, F = x.shape
    n_mol = psi.numel() if n_mol is None else n_mol
    out = torch.full((N_, F), 7.0, device=x.device)
    L = _lib.lib()
    ws_bytes = int(L.spk_eembed_workspace_bytes(N_, n_mol))
    assert ws_bytes >= 0
    work = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    ptrs = (ctypes.c_void_p * len(ws))(*[w.data_ptr() for w in ws])
    _lib.check(L.spk_eembed_fwd_f32(fptr(x) if N_ else None, fptr(psi), iptr(idx_m) if N_ else None, N_, n_mol, F, (len(ws) - 5) // 2, act_id, 1 if charged else 0,
                                    eps, 1 if add_input else 0, ptrs, fptr(out) if N_ else None, ctypes.c_void_p(work.data_ptr()), stream()))
    torch.cuda.synchronize()
    return out


def op_embed(c, add_input, x=None, psi=None, idx=None):
    return torch.ops.spk_hip.electronic_embedding(c["xd"] if x is None else x, c["psid"] if psi is None else psi, c["idxd"] if idx is None else idx, c["wd"],
                                                  c["charged"], c["act_id"], EO.EPS, add_input)


def mirror(c, dev, act=None):
    emb = N.ElectronicEmbedding("psi", c["F"], c["charged"], num_residual=c["n_res"], activation=ACTS[act or c["act"]], epsilon=EO.EPS)
    with torch.no_grad():
        for p, w in zip(emb.operator_weights(), c["ws"]):
            p.copy_(torch.tensor(w))
    return emb.to(dev).eval()


def judge(what, c, out, added):
    """``out`` [N, F] against the fixture (its rows) and the oracle (every row); ``added``: the tensor is x + out."""
    got = out.detach().cpu().double().numpy()
    x64 = c["x"].astype(np.float64)
    ref_all = c["oracle"] + x64 if added else c["oracle"]
    ref_fix = c["want"] + x64[c["rows"]] if added else c["want"]
    e_fix, e_all = EO.rel(got[c["rows"]], ref_fix), EO.rel(got, ref_all)
    bound = TOL if added else c["bound"]
    print("eembed %-34s fixture %.3e  oracle %.3e  (bound %.1e)" % (what, e_fix, e_all, bound))
    assert np.isfinite(got).all() and e_fix <= bound and e_all <= bound, (what, e_fix, e_all, bound)


@pytest.mark.parametrize("name", sorted(EO.CASES))
def test_operator_cases_through_every_route(name, dev):
    c = case(name, dev)
    y_c = c_embed(c["xd"], c["psid"], c["idxd"], c["wd"], c["charged"], c["act_id"])
    if name == "gap":                                              # (every atom belongs to a molecule: nothing of the 7.0 fill is left)
        assert not bool((y_c == 7.0).all(dim=1).any())
    judge(name + " C ABI", c, y_c, False)
    judge(name + " C ABI add_input", c, c_embed(c["xd"], c["psid"], c["idxd"], c["wd"], c["charged"], c["act_id"], add_input=True), True)
    y_op, z_op = op_embed(c, False), op_embed(c, True)
    assert torch.equal(y_op, y_c)                                  # one kernel sequence behind both
    judge(name + " operator", c, y_op, False)
    judge(name + " operator add_input", c, z_op, True)
    emb = mirror(c, dev)
    inp = {"psi": c["psid"], properties.idx_m: c["idxd"]}
    n0 = fallback_count()
    with torch.no_grad():
        y_m, z_m = emb(c["xd"], inp), emb.add_to(c["xd"], inp)
    assert fallback_count() == n0 and emb.on_operator(c["xd"], c["psid"])
    assert torch.equal(y_m, y_op) and torch.equal(z_m, z_op)
    judge(name + " mirror", c, y_m, False)
    neutral = (c["psid"] == 0)[c["idxd"]]
    if bool(neutral.any()):                                        # a neutral molecule: exact zeros, and x itself with add_input
        assert float(y_op[neutral].abs().max()) == 0.0 and torch.equal(z_op[neutral], c["xd"][neutral])
    if name.startswith("pairs"):                                   # the case tells the formula from the one without the eps term
        miss = EO.rel(EO.embedding(c["x"], c["psi"], c["idx_m"], c["ws"], c["charged"], c["act"], eps_term=False)[c["rows"]], c["want"])
        print("eembed %s: the oracle without the eps term misses the fixture by %.2e" % (name, miss))
        assert miss > TOL


@pytest.mark.parametrize("n", [0, 31, 32, 33])
def test_tile_edges_in_the_atom_count(n, dev):
    c = case("edges", dev)
    x, idx, psi = c["xd"][:n].contiguous(), torch.zeros(n, dtype=torch.long, device=dev), torch.tensor([-2.0], device=dev)
    y = op_embed(c, False, x, psi, idx)
    z = c_embed(x, psi, idx, c["wd"], True, c["act_id"], add_input=True)
    assert y.shape == (n, 64)
    if n == 0:
        return
    ref = EO.embedding(c["x"][:n], [-2.0], np.zeros(n, dtype=np.int64), c["ws"], True, c["act"])
    e_y, e_z = EO.rel(y, ref), EO.rel(z, ref + c["x"][:n])
    print("eembed N = %d: out %.3e, x + out %.3e" % (n, e_y, e_z))
    assert e_y <= TOL and e_z <= TOL


def test_two_calls_give_equal_bits_and_at_most_three_launches(dev):
    for name in ("edges", "pairs", "wide"):
        c = case(name, dev)
        a, b = op_embed(c, True), op_embed(c, True)
        assert torch.equal(a, b), name
    c = case("edges", dev)
    _lib.profile_enable(True)
    _lib.profile_report()
    try:
        op_embed(c, True)
        torch.cuda.synchronize()
        prof = _lib.profile_report()
    finally:
        _lib.profile_enable(False)
    print("eembed launches:", {k: v[0] for k, v in prof.items()})
    assert set(prof) == TAGS and all(v[0] == 1 for v in prof.values()), prof


def _lower_bound(idx, key):
    """The kernel's bisection on the host."""
    lo, hi = 0, len(idx)
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if idx[mid] < key:
            lo = mid + 1
        else:
            hi = mid
    return lo


def test_unordered_and_out_of_range_idx_m(dev):
    c = case("edges", dev)
    good = op_embed(c, False)
    idx = c["idx_m"].copy()
    a, b = 10, 120                                   # an atom of molecule 3 and one of molecule 6 trade places
    assert idx[a] == 3 and idx[b] == 6
    idx[a], idx[b] = 6, 3
    n_mol = len(c["psi"])
    sizes = np.asarray(c["sizes"])
    starts = np.concatenate([[0], np.cumsum(sizes)])
    # (the bisections of the kernel still find every molecule's own range on this list: the test is about the foreign atom inside it)
    assert all(_lower_bound(idx, m) == starts[m] and _lower_bound(idx, m + 1) == starts[m + 1] for m in range(n_mol))
    y = op_embed(c, False, idx=torch.tensor(idx, device=dev))
    touched = torch.tensor(np.isin(c["idx_m"], [3, 6]), device=dev)
    assert bool(torch.isnan(y[touched]).all()) and torch.equal(y[~touched], good[~touched])
    # entries outside [0, n_mol) are never an address: their atoms get NaN, the call returns, the other molecules stay finite
    idx = c["idx_m"].copy()
    idx[0], idx[-1] = -5, 10 ** 12
    y = op_embed(c, False, idx=torch.tensor(idx, device=dev))
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[0]).all()) and bool(torch.isnan(y[-1]).all())
    inner = torch.tensor((c["idx_m"] >= 1) & (c["idx_m"] <= 6), device=dev)
    assert bool(torch.isfinite(y[inner]).all())


@pytest.mark.parametrize("what", ["F48", "five_blocks", "tanh"])
def test_declined_shapes_take_aten(what, dev):
    F, n_res, act = {"F48": (48, 1, "ssp"), "five_blocks": (64, 5, "ssp"), "tanh": (64, 1, "tanh")}[what]
    rng = np.random.default_rng(5)
    sizes = [3, 1, 4]
    idx_m = np.repeat(np.arange(3), sizes)
    x = rng.standard_normal((8, F)).astype(np.float32)
    psi = np.asarray([1.0, -2.0, 0.5], dtype=np.float32)
    shapes = [("linear_q.weight", (F, F)), ("linear_q.bias", (F,)), ("linear_k.weight", (F, 2)), ("linear_v.weight", (F, 2))]
    for b in range(n_res):
        shapes += [("w1_%d" % b, (F, F)), ("w2_%d" % b, (F, F))]
    shapes.append(("wl", (F, F)))
    ps = EO.seeded_parameters(shapes, "declined-" + what)
    c = dict(F=F, charged=True, n_res=n_res, act=act, ws=[ps[k] for k, _ in shapes])
    emb = mirror(c, dev)
    assert emb._act == 0
    xd = torch.tensor(x, device=dev)
    inp = {"psi": torch.tensor(psi, device=dev), properties.idx_m: torch.tensor(idx_m, device=dev)}
    n0 = fallback_count()
    with torch.no_grad():
        y = emb(xd, inp)
    assert fallback_count() == n0 + 1 and not emb.on_operator(xd, inp["psi"])
    ref = EO.embedding(x, psi, idx_m, c["ws"], True, act)
    e, e_sum = EO.rel(y, ref), EO.rel(y.cpu().double().numpy() + x, ref + x)
    print("eembed declined %s on ATen: out %.3e, x + out %.3e" % (what, e, e_sum))
    assert e_sum <= TOL
    if what != "tanh":
        with pytest.raises(RuntimeError, match="spk_eembed_supported"):
            torch.ops.spk_hip.electronic_embedding(xd, inp["psi"], inp[properties.idx_m], [torch.tensor(w, device=dev) for w in c["ws"]], True, 1, EO.EPS, False)


def test_autograd_into_the_eval_output_raises(dev):
    c = case("edges", dev)
    emb = mirror(c, dev)
    x = c["xd"].clone().requires_grad_()
    y = emb(x, {"psi": c["psid"], properties.idx_m: c["idxd"]})
    assert y.requires_grad
    with pytest.raises(RuntimeError, match="training mode"):
        y.sum().backward()
    emb.train()                                                     # ... and the training route has the gradients
    y = emb(x, {"psi": c["psid"], properties.idx_m: c["idxd"]})
    y.square().sum().backward()
    assert all(p.grad is not None for p in emb.parameters()) and x.grad is not None


# ----------------------------------------------------------------------------------------------------------------- models
_MODELS = {}


def model_case(tag, dev):
    if tag not in _MODELS:
        arrs = EO.model_arrays(tag)
        _MODELS[tag] = (arrs, EO.build_model(tag).to(dev).eval())
    return _MODELS[tag]


def judge_model(what, tag, out, arrs):
    rows = EO.rep_rows(tag, len(arrs["Z"]))
    errs = {k: EO.rel(out[k][rows] if k == "scalar_representation" else out[k], G["%s_%s" % (tag, k)]) for k in out}
    print("eembed %-44s" % what, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert all(torch.isfinite(v).all() for v in out.values()) and max(errs.values()) <= TOL, (what, errs)


@pytest.mark.parametrize("tag", ["m1", "m2", "m3", "m4"])
def test_models_through_the_potential(tag, dev):
    arrs, model = model_case(tag, dev)
    assert M.classify_potential(model) == 2
    inp = EO.model_inputs(arrs, torch.float32, dev)
    n0 = fallback_count()
    _lib.profile_enable(True)
    _lib.profile_report()
    try:
        out = dict(model(dict(inp)))
        torch.cuda.synchronize()
        prof = _lib.profile_report()
    finally:
        _lib.profile_enable(False)
    assert fallback_count() == n0
    n_emb = len(model.representation.electronic_embeddings)
    print("eembed %s launches:" % tag, {k: v[0] for k, v in prof.items()})
    assert all(prof.get(t, (0,))[0] == n_emb for t in TAGS)          # three launches per embedding
    if tag in ("m1", "m4"):                                          # groups of at most 32 atoms: the molecule-resident launches
        assert {"schnet_mol_fwd", "schnet_mol_bwd"} <= set(prof), prof
    if tag == "m4":                                                  # the rows are looked up inside the first launch
        assert M.embedding_table(model.representation) is not None and not (TAGS & set(prof))
    judge_model(tag + " through NeuralNetworkPotential", tag, EO.run_model(model, inp, EO.MODEL_KEYS[tag]), arrs)
    judge_model(tag + " (the fused call's own outputs)", tag, {k: out[k] for k in ("energy", "forces")}, arrs)


def test_m1_through_the_reference_potential_after_install(dev):
    import types
    from oracle import refshim
    from schnetpack_amd import install
    if not refshim.available():
        pytest.skip("reference (oracle/_ref) not built")
    ns = refshim.load()
    arrs = EO.model_arrays("m1")
    install.install()
    try:
        assert ns.nn.ElectronicEmbedding is N.ElectronicEmbedding and ns.schnet.SchNet.__module__.startswith("schnetpack_amd")
        spk = types.SimpleNamespace(nn=ns.nn, model=ns.model, representation=types.SimpleNamespace(SchNet=ns.schnet.SchNet, PaiNN=ns.painn.PaiNN),
                                    atomistic=types.SimpleNamespace(PairwiseDistances=ns.distances.PairwiseDistances, Atomwise=ns.atomwise.Atomwise,
                                                                    Forces=ns.response.Forces))
        model = EO.build_model("m1", spk).to(dev).eval()
        assert type(model).__module__.startswith("schnetpack.") and M.classify_potential(model) == 2
        inp = EO.model_inputs(arrs, torch.float32, dev)
        inp.pop("_n_molecules")
        out = model(inp)
        out = {k: out[k].detach() for k in ("energy", "forces")}
    finally:
        install.uninstall()
    judge_model("m1 through the reference's NeuralNetworkPotential", "m1", out, arrs)


def test_m1_graphed_force_call_follows_the_charge(dev):
    from schnetpack_amd.forcecall import GraphedForceCall
    arrs, model = model_case("m1", dev)
    inp = EO.model_inputs(arrs, torch.float32, dev)
    call = GraphedForceCall(model)
    first = {k: v.clone() for k, v in call(inp).items()}
    assert call.graph is not None
    eager = model(dict(inp))
    assert EO.rel(first["energy"], eager["energy"]) <= 1e-6 and EO.rel(first["forces"], eager["forces"]) <= 1e-6
    judge_model("m1 graphed", "m1", first, arrs)
    inp["total_charge"].copy_(torch.tensor([-2.0, 0.0, 1.0, 3.0], device=dev))          # in place: the captured launches read it again
    inp["spin_multiplicity"].copy_(torch.tensor([1.0, 2.0, 0.0, 1.5], device=dev))
    again = {k: v.clone() for k, v in call.replay().items()}
    eager = model(dict(inp))
    e_E, e_F = EO.rel(again["energy"], eager["energy"]), EO.rel(again["forces"], eager["forces"])
    moved = EO.rel(again["energy"], first["energy"])
    print("eembed graphed m1 after a change of charge and spin: E %.2e, F %.2e against eager; the energies moved by %.2e" % (e_E, e_F, moved))
    assert e_E <= 1e-6 and e_F <= 1e-6 and moved > 1e-3


def test_so3net_with_a_charge_embedding_against_its_aten_route(dev):
    from schnetpack_amd import atomistic as A, representation as R
    arrs = EO.model_arrays("m1")
    rep = R.SO3net(64, 2, 2, N.GaussianRBF(20, 5.0), N.CosineCutoff(5.0), electronic_embeddings=[N.ElectronicEmbedding("total_charge", 64, True)])
    model = M.NeuralNetworkPotential(rep, input_modules=[A.PairwiseDistances()], output_modules=[A.Atomwise(64, output_key="energy"), A.Forces()])
    model = EO.load_seeded(model, "so3").to(dev).eval()
    emb = rep.electronic_embeddings[0]
    inp = EO.model_inputs(arrs, torch.float32, dev)
    _lib.profile_enable(True)
    _lib.profile_report()
    try:
        hip = {k: v.detach().clone() for k, v in model(dict(inp)).items()}
        torch.cuda.synchronize()
        prof = _lib.profile_report()
    finally:
        _lib.profile_enable(False)
    assert TAGS <= set(prof)
    emb.force_aten = True
    n0 = fallback_count()
    aten = {k: v.detach().clone() for k, v in model(dict(inp)).items()}
    assert fallback_count() > n0
    errs = {k: EO.rel(hip[k], aten[k]) for k in ("energy", "forces")}
    print("eembed SO3net, operator against ATen embedding:", " ".join("%s %.2e" % kv for kv in errs.items()))
    assert max(errs.values()) <= TOL and float(hip["forces"].abs().max()) > 0
