"""Tensorial heads, host side (no device): the float64 restatement (tests/tensorial_oracle.py) and the module mirrors on their ATen route
against the fixture the reference's own code produced (tests/golden/tensorial_cases.npz, tests/make_tensorial_golden.py), the reference's
``state_dict`` layout, TorchScript, which heads the one-launch kernel covers, the classification of a potential with such heads behind it, the
fused routes on the meta device, the names ``install()`` patches and the refusal of the deployed-file export."""
import os
import sys
import types
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tensorial_oracle as TO  # noqa: E402

from schnetpack_amd import _lib, deploy, install as I, model as M, nn as N, properties, torchops  # noqa: E402
from schnetpack_amd.atomistic import (Aggregation, Atomwise, DipoleMoment, Forces, PairwiseDistances, Polarizability, Strain,  # noqa: E402
                                      ZBLRepulsionEnergy)
from schnetpack_amd.nn import CosineCutoff, GaussianRBF  # noqa: E402
from schnetpack_amd.representation import PaiNN, SchNet  # noqa: E402

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tensorial_cases.npz"))
TIGHT = 1.0e-12


def rel(x, ref):
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(np.asarray(x, dtype=np.float64) - ref).max() / (scale if scale > 0 else 1.0))


def head_kwargs(tag):
    n_in, n_layers, n_hidden = TO.CASES[tag]
    return dict(n_in=n_in, n_layers=n_layers, n_hidden=n_hidden if n_hidden else None)


def state_of(keys, weights):
    return {str(k): torch.as_tensor(np.asarray(w), dtype=torch.float32) for k, w in zip(keys, weights)}


def mirror(tag, kind, dtype=torch.float64, **kw):
    """kind 'dv': vector DipoleMoment, 'ds': scalar DipoleMoment, 'pol': Polarizability -- with the fixture's weights (the reference's keys)."""
    c = TO.case_inputs(GOLD, tag)
    wtag = "b" if tag == "c" else tag
    if kind == "ds":
        mod = DipoleMoment(n_in=TO.CASES[tag][0], use_vector_representation=False, **kw)
        mod.load_state_dict(state_of(GOLD[wtag + "_ds_state_keys"], c["ds"]), strict=True)
    elif kind == "dv":
        mod = DipoleMoment(use_vector_representation=True, **head_kwargs(tag), **kw)
        mod.load_state_dict(state_of(GOLD[wtag + "_dv_state_keys"], c["gm"]), strict=True)
    else:
        mod = Polarizability(**head_kwargs(tag), **kw)
        mod.load_state_dict(state_of(GOLD[wtag + "_pol_state_keys"], c["gm"]), strict=True)
    return mod.to(dtype).eval()


def inputs_of(c, dtype=torch.float64, with_q=False, device="cpu"):
    inp = {properties.R: torch.tensor(c["R"], dtype=dtype, device=device), "scalar_representation": torch.tensor(c["s"], dtype=dtype, device=device),
           "vector_representation": torch.tensor(c["v"], dtype=dtype, device=device), properties.idx_m: torch.tensor(c["idx_m"], device=device),
           properties.n_atoms: torch.tensor(c["n_atoms"], device=device), "_n_molecules": torch.tensor(int(c["n_mol"]))}
    if with_q:
        inp[properties.total_charge] = torch.tensor(c["total_charge"], dtype=dtype, device=device)
    return inp


@pytest.mark.parametrize("tag", list(TO.CASES))
def test_restatement_is_pinned_to_the_fixture(tag):
    c = TO.case_inputs(GOLD, tag)
    out = TO.evaluate(c)
    assert ("ds_q" in out) == (tag in ("b", "c"))
    for name, got in out.items():
        assert got.shape == c[name].shape and rel(got, c[name]) < TIGHT, (tag, name)
        # the reference's own float32 gap, recorded by the generator, stays below a quarter of the device tolerance
        assert float(c["gap_" + name]) < 0.25e-5, (tag, name)


def test_the_cases_are_what_their_names_say():
    b, c = TO.case_inputs(GOLD, "b"), TO.case_inputs(GOLD, "c")
    assert list(np.bincount(b["idx_m"], minlength=6)) == [1, 33, 0, 4, 32, 0] and int(b["n_mol"]) == 6 and b["s"].shape == (70, 128)
    assert np.array_equal(b["n_atoms"], np.bincount(b["idx_m"], minlength=6)) and np.all(np.diff(b["idx_m"]) >= 0)
    assert not np.any(c["v"][40]) and np.array_equal(np.delete(c["v"], 40, 0), np.delete(b["v"], 40, 0)) and np.any(b["v"][40])
    assert np.all(b["mu_plain"][[2, 5]] == 0) and np.all(b["alpha"][[2, 5]] == 0)                    # molecules without atoms
    assert np.abs(b["R"]).max() <= 2.5 and TO.case_inputs(GOLD, "a")["s"].shape == (3, 64)
    # corrected charges sum to the requested total
    sums = np.zeros(6)
    np.add.at(sums, b["idx_m"], b["charges_Q"][:, 0])
    assert np.allclose(sums[[0, 1, 3, 4]], b["total_charge"][[0, 1, 3, 4]], atol=1e-12)
    assert np.array_equal(b["alpha"], b["alpha"].transpose(0, 2, 1))


def test_case_a_by_hand():
    """Three atoms, written out without the helpers of the restatement."""
    c = TO.case_inputs(GOLD, "a")
    w = [np.asarray(x, dtype=np.float64) for x in c["gm"]]
    silu = lambda x: x / (1 + np.exp(-x))
    q, mu = np.zeros(3), np.zeros(3)
    d = np.zeros((3, 3))
    for i in range(3):
        s, v = c["s"][i].astype(np.float64), c["v"][i].astype(np.float64)
        for b in range(2):
            wm, w1, b1, w2, b2 = w[5 * b:5 * b + 5]
            m = wm.shape[0] // 2
            mix = np.stack([wm @ v[k] for k in range(3)])
            norm = np.sqrt(mix[0, :m] ** 2 + mix[1, :m] ** 2 + mix[2, :m] ** 2)
            x = w2 @ silu(w1 @ np.concatenate([s, norm]) + b1) + b2
            s, v = (silu(x[:m]) if b == 0 else x[:m]), x[m:][None, :] * mix[:, m:]
        q[i], d[i] = s[0], v[:, 0]
    qc = q - q.sum() / 3
    for i in range(3):
        mu += qc[i] * c["R"][i] + d[i]
    assert rel(mu, c["mu_plain"][0]) < TIGHT and rel(qc, c["charges_plain"][:, 0]) < TIGHT


@pytest.mark.parametrize("tag", list(TO.CASES))
def test_mirrors_on_the_host_in_float64_equal_the_fixture(tag):
    c = TO.case_inputs(GOLD, tag)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, (correct, with_q) in TO.VARIANTS.items():
            out = mirror(tag, "dv", return_charges=True, correct_charges=correct)(inputs_of(c, with_q=with_q))
            assert out[properties.dipole_moment].shape == (int(c["n_mol"]), 3) and out[properties.partial_charges].shape == (c["s"].shape[0], 1)
            assert rel(out[properties.dipole_moment].detach().numpy(), c["mu_" + name]) < TIGHT, (tag, name)
            assert rel(out[properties.partial_charges].detach().numpy(), c["charges_" + name]) < TIGHT, (tag, name)
        out = mirror(tag, "dv", predict_magnitude=True)(inputs_of(c))
        assert properties.partial_charges not in out and rel(out[properties.dipole_moment].detach().numpy(), c["mag_plain"]) < TIGHT
        alpha = mirror(tag, "pol")(inputs_of(c))[properties.polarizability]
        assert alpha.shape == (int(c["n_mol"]), 3, 3) and rel(alpha.detach().numpy(), c["alpha"]) < TIGHT
        s_out, v_out = mirror(tag, "pol").outnet((torch.tensor(c["s"], dtype=torch.float64), torch.tensor(c["v"], dtype=torch.float64)))
        assert rel(s_out.detach().numpy(), c["gm_s"]) < TIGHT and rel(v_out.detach().numpy(), c["gm_v"]) < TIGHT
        if tag in ("b", "c"):              # case f: the scalar DipoleMoment
            for name, (correct, with_q) in TO.VARIANTS.items():
                out = mirror(tag, "ds", return_charges=True, correct_charges=correct)(inputs_of(c, with_q=with_q))
                assert rel(out[properties.dipole_moment].detach().numpy(), c["ds_mu_" + name]) < TIGHT, (tag, name)
                assert rel(out[properties.partial_charges].detach().numpy(), c["ds_charges_" + name]) < TIGHT, (tag, name)
        # without _n_atoms in the batch the atoms are counted from idx_m
        inp = inputs_of(c, with_q=True)
        del inp[properties.n_atoms]
        assert rel(mirror(tag, "dv")(inp)[properties.dipole_moment].detach().numpy(), c["mu_Q"]) < TIGHT


def test_training_mode_has_parameter_and_position_gradients():
    c = TO.case_inputs(GOLD, "a")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for kind, key in (("dv", properties.dipole_moment), ("pol", properties.polarizability)):
            mod = mirror("a", kind).train()
            inp = inputs_of(c)
            inp[properties.R].requires_grad_()
            y = mod(inp)[key]
            assert rel(y.detach().numpy(), c["mu_plain" if kind == "dv" else "alpha"]) < TIGHT
            grads = torch.autograd.grad(y.square().sum(), [inp[properties.R]] + list(mod.parameters()))
            assert all(g is not None and torch.isfinite(g).all() for g in grads) and float(grads[0].abs().max()) > 0


def test_no_atoms_gives_empty_and_zero_outputs_on_the_host():
    """Case d on the ATen route (the reference itself cannot run it: it reads idx_m[-1])."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inp = {properties.R: torch.zeros(0, 3, dtype=torch.float64), "scalar_representation": torch.zeros(0, 64, dtype=torch.float64),
               "vector_representation": torch.zeros(0, 3, 64, dtype=torch.float64), properties.idx_m: torch.zeros(0, dtype=torch.long),
               "_n_molecules": torch.tensor(2)}
        out = mirror("a", "dv", return_charges=True)(dict(inp))
        assert out[properties.partial_charges].shape == (0, 1) and torch.equal(out[properties.dipole_moment], torch.zeros(2, 3, dtype=torch.float64))
        assert torch.equal(mirror("a", "pol")(dict(inp))[properties.polarizability], torch.zeros(2, 3, 3, dtype=torch.float64))


def test_constructors_reproduce_the_reference_state_dict_layout():
    for tag in ("a", "b", "e"):
        for kind, mod in (("dv", DipoleMoment(use_vector_representation=True, **head_kwargs(tag))), ("pol", Polarizability(**head_kwargs(tag)))):
            sd = mod.state_dict()
            assert list(sd) == [str(k) for k in GOLD["%s_%s_state_keys" % (tag, kind)]], (tag, kind)
            for k, shape in zip(sd, GOLD["%s_%s_state_shapes" % (tag, kind)]):
                assert tuple(sd[k].shape) == tuple(int(x) for x in shape[:sd[k].dim()]) and sd[k].dtype == torch.float32, (tag, kind, k)
    sd = DipoleMoment(n_in=128).state_dict()
    assert list(sd) == [str(k) for k in GOLD["b_ds_state_keys"]]
    assert all(tuple(sd[k].shape) == tuple(int(x) for x in s[:sd[k].dim()]) for k, s in zip(sd, GOLD["b_ds_state_shapes"]))
    blk = N.GatedEquivariantBlock(n_sin=8, n_vin=6, n_sout=3, n_vout=5, n_hidden=7)
    assert {k: tuple(v.shape) for k, v in blk.state_dict().items()} == {
        "mix_vectors.weight": (10, 6), "scalar_net.0.weight": (7, 13), "scalar_net.0.bias": (7,), "scalar_net.1.weight": (8, 7), "scalar_net.1.bias": (8,)}
    assert (blk.n_sin, blk.n_vin, blk.n_sout, blk.n_vout, blk.n_hidden, blk.sactivation) == (8, 6, 3, 5, 7, None)
    net = N.build_gated_equivariant_mlp(n_in=32, n_out=2, n_hidden=[20, 12], n_gating_hidden=9, n_layers=3)
    assert [(b.n_sin, b.n_sout, b.n_hidden) for b in net] == [(32, 20, 9), (20, 12, 9), (12, 2, 9)]
    assert [b.sactivation is None for b in net] == [False, False, True] and isinstance(net, torch.nn.Sequential)
    # attributes the reference's classes carry
    d = DipoleMoment(n_in=64, predict_magnitude=True, return_charges=True, dipole_key="mu", charges_key="q", correct_charges=False, use_vector_representation=True)
    assert (d.dipole_key, d.charges_key, d.return_charges, d.predict_magnitude, d.correct_charges, d.use_vector_representation) == ("mu", "q", True, True, False, True)
    assert d.model_outputs == ["mu", "q"] and DipoleMoment(n_in=64).model_outputs == [properties.dipole_moment]
    p = Polarizability(n_in=64, polarizability_key="al")
    assert (p.n_in, p.n_layers, p.n_hidden, p.polarizability_key, p.model_outputs, p.requires_dr, p.requires_stress) == (64, 2, None, "al", ["al"], False, False)
    assert (properties.dipole_moment, properties.polarizability, properties.total_charge, properties.partial_charges) == (
        "dipole_moment", "polarizability", "total_charge", "partial_charges")


def test_which_heads_the_one_launch_kernel_covers():
    lib = _lib.lib()
    assert lib.spk_gated_mlp_supported(64, 2, _lib.SPK_ACT_SILU) == 1 and lib.spk_gated_mlp_supported(128, 2, _lib.SPK_ACT_SILU) == 1
    for n_in, n_layers, act in ((32, 2, _lib.SPK_ACT_SILU), (256, 2, _lib.SPK_ACT_SILU), (128, 3, _lib.SPK_ACT_SILU), (128, 1, _lib.SPK_ACT_SILU),
                                (128, 2, _lib.SPK_ACT_SSP), (128, 2, _lib.SPK_ACT_NONE)):
        assert lib.spk_gated_mlp_supported(n_in, n_layers, act) == 0, (n_in, n_layers, act)
    mk = lambda **kw: DipoleMoment(use_vector_representation=True, **kw)._gated_act
    assert mk(n_in=128) == _lib.SPK_ACT_SILU and mk(n_in=64) == _lib.SPK_ACT_SILU and Polarizability(n_in=128)._gated_act == _lib.SPK_ACT_SILU
    assert mk(n_in=64, n_layers=3, n_hidden=48) == 0 and mk(n_in=128, n_hidden=64) == _lib.SPK_ACT_SILU            # (64 IS the pyramidal width)
    assert mk(n_in=128, n_hidden=32) == 0 and mk(n_in=32) == 0 and mk(n_in=128, activation=N.shifted_softplus) == 0
    assert Polarizability(n_in=128, n_layers=3)._gated_act == 0
    assert DipoleMoment(n_in=128)._scalar_act == _lib.SPK_ACT_SILU and DipoleMoment(n_in=128)._gated_act == 0
    assert DipoleMoment(n_in=128, n_layers=3)._scalar_act == 0 and DipoleMoment(n_in=20)._scalar_act == 0


@pytest.mark.parametrize("tag", ["b", "e"])
def test_torchscript_of_the_mirrors(tag):
    c = TO.case_inputs(GOLD, tag)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for kind, kw, key in (("dv", dict(return_charges=True), properties.dipole_moment), ("pol", {}, properties.polarizability)) + (
                (("ds", dict(predict_magnitude=True), properties.dipole_moment),) if tag == "b" else ()):
            mod = mirror(tag, kind, **kw)
            sm = torch.jit.script(mod)
            want, got = mod(inputs_of(c, with_q=True)), sm(inputs_of(c, with_q=True))
            assert torch.equal(want[key], got[key]), (tag, kind)
            if kind == "dv":
                assert torch.equal(want[properties.partial_charges], got[properties.partial_charges])
                assert rel(got[key].detach().numpy(), c["mu_Q"]) < TIGHT
        blk = N.GatedEquivariantBlock(8, 8, 4, 4, 8, sactivation=torch.nn.functional.silu).double()
        s, v = torch.randn(5, 8, dtype=torch.float64), torch.randn(5, 3, 8, dtype=torch.float64)
        assert all(torch.equal(x, y) for x, y in zip(blk((s, v)), torch.jit.script(blk)((s, v))))
    # on the meta device the scripted modules take the operators (shape inference without a GPU)
    if tag == "b":
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="meta")
        meta = {properties.R: z(7, 3), "scalar_representation": z(7, 128), "vector_representation": z(7, 3, 128), properties.idx_m: z(7, dt=torch.long),
                "_n_molecules": torch.tensor(3)}
        out = torch.jit.script(mirror("b", "dv", torch.float32, return_charges=True).to("meta"))(dict(meta))
        assert out[properties.dipole_moment].shape == (3, 3) and out[properties.partial_charges].shape == (7, 1)
        assert torch.jit.script(mirror("b", "dv", torch.float32, predict_magnitude=True).to("meta"))(dict(meta))[properties.dipole_moment].shape == (3,)
        assert torch.jit.script(mirror("b", "ds", torch.float32).to("meta"))(dict(meta))[properties.dipole_moment].shape == (3, 3)
        assert torch.jit.script(mirror("b", "pol", torch.float32).to("meta"))(dict(meta))[properties.polarizability].shape == (3, 3, 3)


def test_operators_are_registered_and_refuse_host_tensors():
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    for name in ("gated_mlp", "dipole_moment", "polarizability"):
        assert name in torchops.OPERATORS and hasattr(torch.ops.spk_hip, name)
        assert has("spk_hip::" + name, "CUDA") and has("spk_hip::" + name, "Meta") and has("spk_hip::" + name, "CPU"), name
    for name in ("spk_gated_mlp_supported", "spk_gated_mlp_fwd_f32", "spk_moment_reduce_f32"):
        assert name in _lib.exported_symbols() and hasattr(_lib.lib(), name)
    c = TO.case_inputs(GOLD, "a")
    ws = [torch.as_tensor(np.asarray(w)) for w in c["gm"]]
    idx = torch.zeros(3, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.spk_hip.gated_mlp(torch.randn(3, 64), torch.randn(3, 3, 64), ws, _lib.SPK_ACT_SILU)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.spk_hip.dipole_moment(torch.randn(3, 1), None, torch.randn(3, 3), idx, 1, None, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.spk_hip.polarizability(torch.randn(3, 1), torch.randn(3, 3, 1), torch.randn(3, 3), idx, 1)


# ----------------------------------------------------------------------------------------------------------------- the fused force call
def _tail(n_atom_basis, vector):
    if vector:
        return [DipoleMoment(n_in=n_atom_basis, use_vector_representation=True, return_charges=True), Polarizability(n_in=n_atom_basis)]
    return [DipoleMoment(n_in=n_atom_basis, return_charges=True)]


def _potential(kind, mode, tail=True, n_atom_basis=128):
    rep = (SchNet if kind == "schnet" else PaiNN)(n_atom_basis, 1, GaussianRBF(20, 5.0), CosineCutoff(5.0))
    stress = mode in (3, 5)
    if mode in (4, 5):
        outs = [Atomwise(n_in=n_atom_basis, output_key="e_nn"), ZBLRepulsionEnergy("eV", "Ang", "e_zbl", cutoff_fn=CosineCutoff(4.0)),
                Aggregation(["e_nn", "e_zbl"], properties.energy), Forces(calc_forces=True, calc_stress=stress)]
    else:
        outs = [Atomwise(n_in=n_atom_basis, output_key=properties.energy), Forces(calc_forces=True, calc_stress=stress)]
    if tail:
        outs = outs + _tail(n_atom_basis, kind == "painn")
    return M.NeuralNetworkPotential(rep, input_modules=([Strain()] if stress else []) + [PairwiseDistances()], output_modules=outs)


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_classification_with_a_tensorial_tail(kind):
    n_tail = 2 if kind == "painn" else 1
    for mode in (2, 3, 4, 5):
        with_tail, without = _potential(kind, mode), _potential(kind, mode, tail=False)
        assert M.classify_potential(with_tail) == mode and M.classify_potential(without) == mode, mode
        assert with_tail._n_tail == n_tail and without._n_tail == 0 and M.tensorial_tail(list(without.output_modules)) == 0
        assert (with_tail._potential_forces, with_tail._potential_stress, with_tail._potential_zbl, with_tail._zbl_stress) == (
            without._potential_forces, without._potential_stress, without._potential_zbl, without._zbl_stress)
        assert with_tail._zbl_layout == without._zbl_layout == ([0, 1, 2, 3] if mode in (4, 5) else [])
        assert properties.dipole_moment in with_tail.model_outputs and properties.partial_charges in with_tail.model_outputs
        assert properties.dipole_moment not in without.model_outputs
        # training: the force-matching engine is for the bare potential only
        assert with_tail._fm_head_act == 0 and not with_tail.fm_engine and (without.fm_engine == (mode == 2))
    # a tensorial head anywhere but at the end: module by module
    for mode in (2, 4):
        m = _potential(kind, mode, tail=False)
        outs = list(m.output_modules)
        moved = M.NeuralNetworkPotential(m.representation, input_modules=list(m.input_modules), output_modules=outs[:-1] + _tail(128, kind == "painn")[:1] + outs[-1:])
        assert M.classify_potential(moved) == 0 and moved._n_tail == 0
    # energy only (+ tail): SchNet keeps its one-operator energy, PaiNN has no such form -- as without the tail
    rep = _potential(kind, 2).representation
    only_e = M.NeuralNetworkPotential(rep, input_modules=[PairwiseDistances()], output_modules=[Atomwise(n_in=128)] + _tail(128, kind == "painn"))
    assert M.classify_potential(only_e) == (0 if kind == "painn" else 1)
    # a subclass is not the mirror: it may compute something else
    class Mine(Polarizability):
        pass
    m = _potential(kind, 2, tail=False)
    sub = M.NeuralNetworkPotential(m.representation, input_modules=[PairwiseDistances()], output_modules=list(m.output_modules) + [Mine(n_in=128)])
    assert M.classify_potential(sub) == 0


def _meta_batch(N=12, E=40, n_mol=2):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="meta")
    return {properties.Z: z(N, dt=torch.long), properties.R: z(N, 3), properties.idx_i: z(E, dt=torch.long), properties.idx_j: z(E, dt=torch.long),
            properties.offsets: z(E, 3), properties.idx_m: z(N, dt=torch.long), properties.cell: z(n_mol, 3, 3), "_n_molecules": torch.tensor(n_mol)}


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_whole_force_call_with_a_tail_on_the_meta_device(kind):
    d = _meta_batch()
    for mode in (2, 3, 4, 5):
        m = _potential(kind, mode).to("meta").eval()
        for model in (m, torch.jit.script(m)):
            out = model(dict(d))
            assert out[properties.energy].shape == (2,) and out[properties.forces].shape == (12, 3) and (properties.stress in out) == (mode in (3, 5))
            assert out[properties.dipole_moment].shape == (2, 3) and out[properties.partial_charges].shape == (12, 1)
            assert (out[properties.polarizability].shape == (2, 3, 3)) if kind == "painn" else (properties.polarizability not in out)
        assert set(m(dict(d))) == set(m.model_outputs)


def test_install_routes_a_reference_model_with_a_tail_through_the_fused_call():
    """``install._fused_potential_call`` around a stand-in for the reference's ``NeuralNetworkPotential`` (model/base.py:132-190): the tail runs
    behind the fused route (the stand-in's own forward would raise), on the meta device."""
    class RefModel(torch.nn.Module):
        def __init__(self, src):
            super().__init__()
            self.representation, self.input_modules, self.output_modules = src.representation, src.input_modules, src.output_modules
            self.model_outputs, self.required_derivatives = src.model_outputs, src.required_derivatives

        def initialize_derivatives(self, inputs):
            for p in self.required_derivatives:
                if p in inputs:
                    inputs[p].requires_grad_()
            return inputs

        def postprocess(self, inputs):
            return inputs

        def extract_outputs(self, inputs):
            return {k: inputs[k] for k in self.model_outputs}

        def forward(self, inputs):
            raise AssertionError("the reference's own forward ran")

    RefModel.__call__ = I._fused_potential_call(torch.nn.Module.__call__)
    d = _meta_batch()
    for kind in ("schnet", "painn"):
        for mode in (2, 3, 4, 5):
            ref = RefModel(_potential(kind, mode)).to("meta").eval()
            out = ref(dict(d))
            assert ref.__dict__["_spk_hip_mode"] == mode and ref.__dict__["_spk_hip_tail"] == (2 if kind == "painn" else 1)
            assert out[properties.energy].shape == (2,) and out[properties.forces].shape == (12, 3) and out[properties.dipole_moment].shape == (2, 3)
            assert (properties.polarizability in out) == (kind == "painn")
            bare = RefModel(_potential(kind, mode, tail=False)).to("meta").eval()
            assert set(bare(dict(d))) == set(bare.model_outputs) and bare.__dict__["_spk_hip_tail"] == 0 and bare.__dict__["_spk_hip_mode"] == mode
    # mode 1 (SchNet, energy only): the module loop of that route already runs the tail
    rep = _potential("schnet", 2).representation
    ref = RefModel(M.NeuralNetworkPotential(rep, input_modules=[PairwiseDistances()], output_modules=[Atomwise(n_in=128)] + _tail(128, False))).to("meta").eval()
    out = ref(dict(d))
    assert ref.__dict__["_spk_hip_mode"] == 1 and out[properties.dipole_moment].shape == (2, 3)


def test_install_patches_the_new_names_and_uninstall_restores_them():
    class RefBlock:
        pass

    class RefDipole:
        pass

    class RefPol:
        pass

    def ref_build():
        pass

    pkg = types.ModuleType("spkstub2")
    subs = {}
    for name, attrs in (("nn", dict(GatedEquivariantBlock=RefBlock, build_gated_equivariant_mlp=ref_build)),
                        ("nn.equivariant", dict(GatedEquivariantBlock=RefBlock)),
                        ("nn.blocks", dict(build_gated_equivariant_mlp=ref_build)),
                        ("atomistic", dict(DipoleMoment=RefDipole, Polarizability=RefPol)),
                        ("atomistic.atomwise", dict(DipoleMoment=RefDipole, Polarizability=RefPol))):
        mod = types.ModuleType("spkstub2." + name)
        mod.__dict__.update(attrs)
        subs[name] = sys.modules["spkstub2." + name] = mod
    pkg.nn, pkg.atomistic = subs["nn"], subs["atomistic"]
    bare = types.ModuleType("spkstub3")                       # a reference that has not loaded these modules is left alone
    bare.nn = types.ModuleType("spkstub3.nn")
    try:
        log = I.install(pkg)
        for want in ("spkstub2.nn.GatedEquivariantBlock", "spkstub2.nn.equivariant.GatedEquivariantBlock", "spkstub2.nn.build_gated_equivariant_mlp",
                     "spkstub2.nn.blocks.build_gated_equivariant_mlp", "spkstub2.atomistic.DipoleMoment", "spkstub2.atomistic.atomwise.DipoleMoment",
                     "spkstub2.atomistic.Polarizability", "spkstub2.atomistic.atomwise.Polarizability"):
            assert want in log, want
        assert subs["nn"].GatedEquivariantBlock is N.GatedEquivariantBlock and subs["nn.equivariant"].GatedEquivariantBlock is N.GatedEquivariantBlock
        assert subs["nn"].build_gated_equivariant_mlp is N.build_gated_equivariant_mlp and subs["nn.blocks"].build_gated_equivariant_mlp is N.build_gated_equivariant_mlp
        assert subs["atomistic"].DipoleMoment is DipoleMoment and subs["atomistic.atomwise"].Polarizability is Polarizability
        assert not any("Gated" in x or "Dipole" in x for x in I.install(bare)) and not hasattr(bare.nn, "GatedEquivariantBlock")
        I.uninstall()
        assert subs["nn"].GatedEquivariantBlock is RefBlock and subs["nn.equivariant"].GatedEquivariantBlock is RefBlock
        assert subs["nn"].build_gated_equivariant_mlp is ref_build and subs["nn.blocks"].build_gated_equivariant_mlp is ref_build
        assert subs["atomistic"].DipoleMoment is RefDipole and subs["atomistic.atomwise"].DipoleMoment is RefDipole
        assert subs["atomistic"].Polarizability is RefPol and subs["atomistic.atomwise"].Polarizability is RefPol
    finally:
        I.uninstall()
        for name in subs:
            sys.modules.pop("spkstub2." + name, None)


def test_export_refuses_a_model_with_a_tensorial_head_and_names_it():
    for kind, name in (("painn", "DipoleMoment"), ("schnet", "DipoleMoment")):
        with pytest.raises(ValueError, match="tensorial head \\(%s\\)" % name):
            deploy.export_potential(_potential(kind, 2).eval())
    m = _potential("painn", 2, tail=False)
    only_pol = M.NeuralNetworkPotential(m.representation, input_modules=[PairwiseDistances()], output_modules=list(m.output_modules) + [Polarizability(n_in=128)])
    with pytest.raises(ValueError, match="Polarizability"):
        deploy.export_potential(only_pol.eval())
    assert len(deploy.export_potential(m.eval())) > 0
