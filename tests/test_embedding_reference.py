"""CPU: the charge / spin embeddings against the fixture the reference's own classes produced (tests/golden/embedding_cases.npz,
tests/make_embedding_golden.py).

  * the numpy oracle (tests/embedding_oracle.py: the per-molecule formula exp(w - M_m) / (S_m + eps Z exp(M - M_m))) reproduces every operator
    case to 1e-12, agrees with the reference's own order of operations, and misses the ``pairs`` cases by more than 1e-5 without the eps term;
  * the mirrors on their ATen route in float64 meet the operator and the model cases within 1e-10;
  * ``state_dict`` keys and shapes are the fixture's (the reference's), and the reference's own dict loads strictly where it can be imported;
  * ``NuclearEmbedding``: eval table against the fixture, the configuration table against the live reference, ``max_z != 101`` raises;
  * ``install()`` routes the five classes, ``uninstall()`` restores them;
  * the operator on Meta tensors, its refusal of host tensors, ``spk_eembed_supported``;
  * training mode gives every parameter a gradient; routing flags of declined shapes;
  * ``export_potential``: plain models byte for byte as before, a ``NuclearEmbedding`` model exports its eval table, electronic embeddings are refused.
"""
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import embedding_oracle as EO  # noqa: E402

from schnetpack_amd import _lib, nn as N, properties  # noqa: E402
from schnetpack_amd.nn import embedding as E  # noqa: E402

ORACLE_TOL = 1.0e-12
HOST_TOL = 1.0e-10
G = EO.gold()
ACTS = {"ssp": N.shifted_softplus, "silu": torch.nn.functional.silu}


def mirror(c, dtype=torch.float64):
    """The mirror of an operator case with the case's weights (the operator's weight order is the module's parameter order)."""
    emb = N.ElectronicEmbedding("psi", c["F"], c["charged"], num_residual=c["n_res"], activation=ACTS[c["act"]], epsilon=EO.EPS)
    with torch.no_grad():
        for p, w in zip(emb.operator_weights(), c["ws"]):
            p.copy_(torch.tensor(w))
    return emb.to(dtype)


def inputs_of(c, dtype, dev="cpu"):
    return {"psi": torch.tensor(c["psi"], dtype=dtype, device=dev), properties.idx_m: torch.tensor(c["idx_m"], device=dev)}


@pytest.mark.parametrize("name", sorted(EO.CASES))
def test_oracle_reproduces_the_fixture(name):
    c = EO.check_streams(G, name)
    want, rows = EO.expected(G, name)
    out, alpha = EO.embedding(c["x"], c["psi"], c["idx_m"], c["ws"], c["charged"], c["act"], return_alpha=True)
    err = EO.rel(out[rows], want)
    w = EO.logits(c["x"], c["psi"], c["idx_m"], c["ws"], c["charged"])
    both = float(np.abs(alpha - EO.attention_batch_softmax(w, c["idx_m"], len(c["psi"]))).max())
    print("%s: oracle against the fixture %.1e; per-molecule form against the batch softmax %.1e" % (name, err, both))
    assert err < ORACLE_TOL and both < ORACLE_TOL
    if name.startswith("pairs"):
        assert float(np.abs(alpha - G[name + "_alpha"]).max()) < ORACLE_TOL
        miss = EO.rel(EO.embedding(c["x"], c["psi"], c["idx_m"], c["ws"], c["charged"], c["act"], eps_term=False)[rows], want)
        print("%s: without the eps term %.1e" % (name, miss))
        assert miss > 1.0e-5                               # the case tells the two formulas apart
    assert float(G[name + "_gap"]) <= (6.0e-6 if name == "silu" else 5.0e-6)


@pytest.mark.parametrize("name", sorted(EO.CASES))
def test_mirror_on_the_aten_route_meets_the_fixture(name):
    c = EO.case(name)
    want, rows = EO.expected(G, name)
    emb = mirror(c).eval()
    x = torch.tensor(c["x"], dtype=torch.float64)
    with torch.no_grad():
        y = emb(x, inputs_of(c, torch.float64))
        z = emb.add_to(x, inputs_of(c, torch.float64))
    err = EO.rel(y[rows], want)
    print("%s: mirror (float64, host) %.1e" % (name, err))
    assert err < HOST_TOL and torch.equal(z, x + y)
    neutral = torch.tensor(c["psi"] == 0)[torch.tensor(c["idx_m"])]
    assert float(y[neutral].abs().max() if neutral.any() else 0.0) < 1e-15


@pytest.mark.parametrize("tag", ["m1", "m2", "m3", "m4"])
def test_mirror_models_on_the_host_meet_the_fixture(tag):
    arrs = EO.model_arrays(tag)
    model = EO.build_model(tag).double().eval()
    ck = EO.checksum([arrs[k] for k in sorted(arrs)] + list(v for _, v in sorted(EO.seeded_parameters(EO.parameter_shapes(model), EO.MODEL_WEIGHTS[tag]).items())))
    assert abs(ck - float(G[tag + "_checksum"])) <= 1e-9 * abs(ck)
    assert [str(k) for k in G[tag + "_sd_keys"]] == list(model.state_dict().keys())
    out = EO.run_model(model, EO.model_inputs(arrs, torch.float64, "cpu"), EO.MODEL_KEYS[tag])
    rows = EO.rep_rows(tag, len(arrs["Z"]))
    errs = {k: EO.rel(out[k][rows] if k == "scalar_representation" else out[k], G["%s_%s" % (tag, k)]) for k in EO.MODEL_KEYS[tag]}
    print(tag, " ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) < HOST_TOL


def _layout(sd):
    return [(k, tuple(v.shape)) for k, v in sd.items()]


def _fixture_layout(prefix):
    return [(str(k), tuple(int(s) for s in shp if s >= 0)) for k, shp in zip(G[prefix + "_keys"], G[prefix + "_shapes"])]


def test_state_dict_layouts_are_the_reference_s():
    ssp = N.shifted_softplus
    assert _layout(N.ElectronicEmbedding("total_charge", 64, True, num_residual=2).state_dict()) == _fixture_layout("sd_ee")
    assert _layout(N.NuclearEmbedding(101, 64).state_dict()) == _fixture_layout("sd_ne")
    assert _layout(N.Residual(64, ssp).state_dict()) == _fixture_layout("sd_res")
    assert _layout(N.ResidualStack(64, 2, ssp).state_dict()) == _fixture_layout("sd_stack")
    assert _layout(N.ResidualMLP(64, 1, ssp).state_dict()) == _fixture_layout("sd_mlp")
    ne = N.NuclearEmbedding(101, 64)
    assert "embedding" in dict(ne.named_buffers()) and "embedding" not in ne.state_dict()       # non-persistent
    # initialisation: zero table and zero output layer (so a fresh embedding adds nothing), orthogonal q / k / v
    assert float(ne.element_embedding.detach().abs().max()) == 0.0 and float(ne.config_linear.weight.detach().abs().max()) == 0.0
    ee = N.ElectronicEmbedding("total_charge", 64, True)
    assert float(ee.resblock.linear.weight.detach().abs().max()) == 0.0 and float(ee.linear_q.bias.detach().abs().max()) == 0.0
    assert torch.allclose((ee.linear_q.weight @ ee.linear_q.weight.T).detach(), torch.eye(64), atol=1e-5)
    assert properties.spin_multiplicity == "spin_multiplicity" and properties.idx == "_idx" and properties.total_charge == "total_charge"


def test_reference_state_dicts_load_and_the_configuration_table_is_the_reference_s():
    from oracle import refshim
    if not refshim.available():
        pytest.skip("reference sources not available")
    ns = refshim.load()
    ref = ns.nn.ElectronicEmbedding("total_charge", 64, True, num_residual=2)
    N.ElectronicEmbedding("total_charge", 64, True, num_residual=2).load_state_dict(ref.state_dict(), strict=True)
    rne = ns.nn.NuclearEmbedding(101, 64, zero_init=False)
    mine = N.NuclearEmbedding(101, 64)
    mine.load_state_dict(rne.state_dict(), strict=True)
    assert torch.equal(mine.electron_config, rne.electron_config)
    assert np.array_equal(E.electron_config, sys.modules["schnetpack.nn.embedding"].electron_config)
    Z = torch.tensor([1, 6, 8, 26, 79, 92, 100])
    rne.eval()                                          # (the reference's train() returns None)
    assert torch.equal(mine.eval()(Z), rne(Z))
    c = EO.case("edges")
    rm = ns.nn.ElectronicEmbedding("psi", 64, True, num_residual=2)
    mm = mirror(c, torch.float32)
    rm.load_state_dict(mm.state_dict(), strict=True)
    x, inp = torch.tensor(c["x"]), inputs_of(c, torch.float32)
    inp["_idx"] = torch.arange(len(c["psi"]))
    with torch.no_grad():
        assert EO.rel(mm.eval()(x, inp), rm.eval()(x, inp)) < 1e-6


def test_nuclear_embedding_eval_table_and_its_size_check():
    ne = EO.load_seeded(N.NuclearEmbedding(101, 64, zero_init=False), "ne").double()
    ck = EO.checksum(list(EO.seeded_parameters(EO.parameter_shapes(ne), "ne").values()))
    assert abs(ck - float(G["ne_checksum"])) <= 1e-9 * abs(ck)
    assert ne.eval() is ne and ne.train() is ne and ne.train(False) is ne
    assert EO.rel(ne.embedding, G["ne_table"]) < ORACLE_TOL
    Z = torch.tensor([0, 1, 8, 100])
    assert torch.equal(ne(Z), ne.embedding[Z])
    with torch.no_grad():
        ne.element_embedding.add_(1.0)
    assert EO.rel(ne.embedding, G["ne_table"]) < ORACLE_TOL           # eval mode: the table is what it was at the switch
    ne.train()
    assert EO.rel(ne(Z).detach(), G["ne_table"][Z.numpy()] + 1.0) < ORACLE_TOL and ne(Z).requires_grad
    for bad in (100, 102, 10):
        with pytest.raises(ValueError, match="max_z must be 101"):
            N.NuclearEmbedding(bad, 64)
    assert E.electron_config.shape == (101, 23) and E.electron_config.dtype == np.float32 and float(E.electron_config.max()) == 1.0


def test_install_routes_the_five_classes_and_uninstall_restores_them():
    from oracle import refshim
    if not refshim.available():
        pytest.skip("reference sources not available")
    ns = refshim.load()
    from schnetpack_amd import install
    remb, rblk = sys.modules["schnetpack.nn.embedding"], sys.modules["schnetpack.nn.blocks"]
    places = [(ns.nn, n) for n in ("ElectronicEmbedding", "NuclearEmbedding")] + [(remb, n) for n in ("ElectronicEmbedding", "NuclearEmbedding", "ResidualMLP")]
    places += [(rblk, n) for n in ("Residual", "ResidualStack", "ResidualMLP")]
    places += [(ns.nn, n) for n in ("Residual", "ResidualStack", "ResidualMLP") if hasattr(ns.nn, n)]
    before = [getattr(m, n) for m, n in places]
    log = install.install()
    try:
        assert all(getattr(m, n) is getattr(N, n) for m, n in places)
        assert all("%s.%s" % (m.__name__, n) in log for m, n in places)
    finally:
        install.uninstall()
    assert all(getattr(m, n) is b for (m, n), b in zip(places, before))


def test_operator_on_meta_tensors_and_its_refusals():
    c = EO.case("edges")
    emb = mirror(c, torch.float32)
    meta = lambda t: t.to("meta")
    x = torch.tensor(c["x"])
    for add in (False, True):
        y = torch.ops.spk_hip.electronic_embedding(meta(x), meta(torch.tensor(c["psi"])), meta(torch.tensor(c["idx_m"])), [meta(w) for w in emb.operator_weights()],
                                                   True, c["act_id"], EO.EPS, add)
        assert y.is_meta and y.shape == x.shape and y.dtype == torch.float32
    with pytest.raises(RuntimeError):            # no CPU kernel: a host tensor is refused, never computed by a quiet fall-back
        torch.ops.spk_hip.electronic_embedding(x, torch.tensor(c["psi"]), torch.tensor(c["idx_m"]), emb.operator_weights(), True, c["act_id"], EO.EPS, False)
    lib = _lib.lib()
    for F in range(32, 257, 32):
        for r in range(5):
            assert lib.spk_eembed_supported(F, r, _lib.SPK_ACT_SSP) == 1 and lib.spk_eembed_supported(F, r, _lib.SPK_ACT_SILU) == 1
    for F, r, a in ((48, 1, 1), (0, 1, 1), (16, 1, 1), (288, 1, 1), (64, 5, 1), (64, -1, 1), (64, 1, _lib.SPK_ACT_NONE), (64, 1, 3)):
        assert lib.spk_eembed_supported(F, r, a) == 0, (F, r, a)
    assert lib.spk_eembed_workspace_bytes(0, 0) == 0 and lib.spk_eembed_workspace_bytes(-1, 1) < 0
    assert lib.spk_eembed_workspace_bytes(4500, 3000) >= 4 * 4500 + 8 * 18 + 24 * 3000


def test_routing_flags():
    assert N.ElectronicEmbedding("q", 64, True)._act == _lib.SPK_ACT_SSP
    assert N.ElectronicEmbedding("q", 128, False, num_residual=4, activation=torch.nn.functional.silu)._act == _lib.SPK_ACT_SILU
    assert N.ElectronicEmbedding("q", 48, True)._act == 0 and N.ElectronicEmbedding("q", 64, True, num_residual=5)._act == 0
    assert N.ElectronicEmbedding("q", 64, True, activation=torch.tanh)._act == 0
    emb = N.ElectronicEmbedding("q", 64, True).eval()
    assert not emb.on_operator(torch.zeros(3, 64), torch.zeros(1))                         # host tensors
    assert not emb.on_operator(torch.zeros(3, 64, dtype=torch.float64, device="meta"), torch.zeros(1, device="meta"))


def test_training_mode_gives_every_parameter_a_gradient():
    c = EO.case("edges")
    emb = mirror(c, torch.float64).train()
    x = torch.tensor(c["x"], dtype=torch.float64, requires_grad=True)
    y = emb(x, inputs_of(c, torch.float64))
    y.square().sum().backward()
    for k, p in emb.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0.0, k
    assert x.grad is not None and float(x.grad.abs().max()) > 0.0
    ne = N.NuclearEmbedding(101, 64, zero_init=False).train()
    ne(torch.tensor([1, 6, 8])).square().sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0.0 for p in ne.parameters())


def _tensors(blob):
    """{tensor name: float32 array} of a deployed file (layout: schnetpack_amd/deploy.py)."""
    from schnetpack_amd import deploy
    assert blob[:8] == deploy.MAGIC
    n_t = struct.unpack("<16i", blob[8:72])[12]
    data0 = (88 + 48 * n_t + 63) // 64 * 64
    out = {}
    for k in range(n_t):
        o = 88 + 48 * k
        n, off = struct.unpack("<qq", blob[o + 32:o + 48])
        out[blob[o:o + 32].rstrip(b"\0").decode()] = np.frombuffer(blob, dtype="<f4", count=n, offset=data0 + 4 * off)
    return out


def test_export_potential():
    from make_deploy_parent_golden import formula_model
    from schnetpack_amd import deploy, model as M
    before = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deploy_parent_blobs.npz"))
    for kind in ("schnet", "painn"):                   # a plain model: byte for byte the file written before the embeddings existed
        assert deploy.export_potential(formula_model(kind)) == before["formula_" + kind].tobytes(), kind
    m4 = EO.build_model("m4").eval()
    assert M.classify_potential(m4) == 2 and M.embedding_table(m4.representation) is m4.representation.embedding.embedding
    ts = _tensors(deploy.export_potential(m4))
    ne = m4.representation.embedding
    assert np.array_equal(ts["embedding"].reshape(101, 128), (ne.element_embedding + ne.config_linear(ne.electron_config)).detach().numpy())
    assert np.array_equal(ts["embedding"].reshape(101, 128), ne.embedding.numpy())
    m4.train()
    assert M.embedding_table(m4.representation) is None                      # training mode: the rows are recomputed by the module
    for tag in ("m1", "m3"):
        m = EO.build_model(tag).eval()
        assert M.classify_potential(m) == 2 and M.embedding_table(m.representation) is None and M.classify_fm(m) == 0
        with pytest.raises(ValueError, match="electronic embeddings are not supported"):
            deploy.export_potential(m)
