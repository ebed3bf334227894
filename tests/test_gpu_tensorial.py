"""GPU: the tensorial heads (csrc/spk_tensorial.hip) through every route -- the C ABI, ``torch.ops.spk_hip.{gated_mlp, dipole_moment,
polarizability}``, the module mirrors, the fused force call with the heads behind it, the reference's own classes on the mirrors -- against the
float64 fixture the reference's own code produced (tests/golden/tensorial_cases.npz, tests/make_tensorial_golden.py).

Tolerance: the project's parity contract, ``max|a - b| / max|b| <= 1e-5``, on s_out, v_out, charges, mu and alpha, with no
extra margin; the reference's own float32 gap on these cases is below a quarter of it (``gap_*`` in the fixture).  Every test prints what it
measured.
"""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tensorial_oracle as TO  # noqa: E402

from oracle import refshim  # noqa: E402
from schnetpack_amd import _lib, model as M, properties, synthetic as S  # noqa: E402
from schnetpack_amd._lib import SpkHipError, fptr, iptr, stream  # noqa: E402
from schnetpack_amd.atomistic import Atomwise, DipoleMoment, Forces, PairwiseDistances, Polarizability, Strain  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1.0e-5
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tensorial_cases.npz"))
FUSED = ["a", "b", "c"]
SILU = _lib.SPK_ACT_SILU
DIPOLE, POLAR = 0, 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    return torch.device("cuda", 0)


def rel(x, ref):
    ref = np.asarray(ref, dtype=np.float64)
    x = x.detach().cpu().double().numpy() if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(x.reshape(ref.shape) - ref).max() / (scale if scale > 0 else 1.0))


def check(what, got, want):
    e = rel(got, want)
    print("tensorial %-34s %.3e" % (what, e))
    assert torch.isfinite(got).all() and e <= TOL, (what, e)


_CASES = {}


def case(tag, dev):
    """Fixture case on the device (built once, never modified): arrays, the float32 batch dict, the weight lists."""
    if tag not in _CASES:
        c = TO.case_inputs(GOLD, tag)
        t = lambda k, dt: torch.tensor(c[k], dtype=dt, device=dev)
        inp = {properties.R: t("R", torch.float32), "scalar_representation": t("s", torch.float32), "vector_representation": t("v", torch.float32),
               properties.idx_m: t("idx_m", torch.long), properties.n_atoms: t("n_atoms", torch.long), "_n_molecules": int(c["n_mol"])}
        gm = [torch.tensor(np.asarray(w), dtype=torch.float32, device=dev) for w in c["gm"]]
        ds = [torch.tensor(np.asarray(w), dtype=torch.float32, device=dev) for w in c.get("ds", [])]
        _CASES[tag] = (c, inp, gm, ds, t("total_charge", torch.float32))
    return _CASES[tag]


def batch(inp, total=None):
    d = dict(inp)
    if total is not None:
        d[properties.total_charge] = total
    return d


def mirror(tag, kind, dev, **kw):
    c = TO.case_inputs(GOLD, tag)
    wtag = "b" if tag == "c" else tag
    n_in, n_layers, n_hidden = TO.CASES[tag]
    hk = dict(n_in=n_in, n_layers=n_layers, n_hidden=n_hidden if n_hidden else None)
    if kind == "ds":
        mod, keys, ws = DipoleMoment(n_in=n_in, use_vector_representation=False, **kw), GOLD[wtag + "_ds_state_keys"], c["ds"]
    elif kind == "dv":
        mod, keys, ws = DipoleMoment(use_vector_representation=True, **hk, **kw), GOLD[wtag + "_dv_state_keys"], c["gm"]
    else:
        mod, keys, ws = Polarizability(**hk, **kw), GOLD[wtag + "_pol_state_keys"], c["gm"]
    mod.load_state_dict({str(k): torch.as_tensor(np.asarray(w), dtype=torch.float32) for k, w in zip(keys, ws)}, strict=True)
    return mod.to(dev).eval()


# ----------------------------------------------------------------------------------------------------------------- C ABI
def c_gated(s, v, ws, n_layers=2):
    N, F = s.shape
    so, vo = torch.full((N, 1), 7.0, device=s.device), torch.full((N, 3, 1), 7.0, device=s.device)
    ptrs = (ctypes.c_void_p * len(ws))(*[w.data_ptr() for w in ws])
    _lib.check(_lib.lib().spk_gated_mlp_fwd_f32(fptr(s) if N else None, fptr(v) if N else None, N, F, n_layers, SILU, ptrs, fptr(so) if N else None,
                                                fptr(vo) if N else None, stream()))
    return so, vo


def c_moment(kind, q, d, R, idx_m, n_mol, total=None, correct=True, want_q=True):
    N = R.shape[0]
    out = torch.full((n_mol, 3) if kind == DIPOLE else (n_mol, 3, 3), 7.0, device=R.device)
    qo = torch.full((N, 1), 7.0, device=R.device) if (kind == DIPOLE and want_q) else None
    p = lambda t: fptr(t) if (t is not None and t.numel()) else None
    _lib.check(_lib.lib().spk_moment_reduce_f32(kind, p(q), p(d), p(R), iptr(idx_m) if N else None, N, n_mol, p(total), 1 if correct else 0, p(out), p(qo),
                                                stream()))
    return out, qo


@pytest.mark.parametrize("tag", FUSED)
def test_c_abi(dev, tag):
    c, inp, gm, ds, total = case(tag, dev)
    s, v, R, idx_m, n_mol = inp["scalar_representation"], inp["vector_representation"], inp[properties.R], inp[properties.idx_m], int(c["n_mol"])
    so, vo = c_gated(s, v, gm)
    check(tag + " c-abi s_out", so, c["gm_s"])
    check(tag + " c-abi v_out", vo, c["gm_v"])
    assert not (so == 7.0).any() and not (vo == 7.0).any()                      # every element written
    so2, vo2 = c_gated(s, v, gm)
    assert torch.equal(so, so2) and torch.equal(vo, vo2)                         # the same bits on a second call
    d = vo.reshape(-1, 3)
    empty = np.flatnonzero(np.bincount(c["idx_m"], minlength=n_mol) == 0)
    for name, (correct, with_q) in TO.VARIANTS.items():
        mu, qo = c_moment(DIPOLE, so, d, R, idx_m, n_mol, total if with_q else None, correct)
        check("%s c-abi mu_%s" % (tag, name), mu, c["mu_" + name])
        check("%s c-abi charges_%s" % (tag, name), qo, c["charges_" + name])
        assert not (qo == 7.0).any() and not (mu == 7.0).any()
        assert torch.equal(mu[empty], torch.zeros(len(empty), 3, device=dev))  # molecules without atoms: exactly zero
        mu2, qo2 = c_moment(DIPOLE, so, d, R, idx_m, n_mol, total if with_q else None, correct)
        assert torch.equal(mu, mu2) and torch.equal(qo, qo2)
    mu_nq, none = c_moment(DIPOLE, so, d, R, idx_m, n_mol, None, True, want_q=False)           # charges not asked for
    assert none is None and rel(mu_nq, c["mu_plain"]) <= TOL
    al, _ = c_moment(POLAR, so, d, R, idx_m, n_mol)
    check(tag + " c-abi alpha", al, c["alpha"])
    assert torch.equal(al, al.transpose(1, 2)) and not (al == 7.0).any()         # alpha == alpha^T to the bit
    assert torch.equal(al[empty], torch.zeros(len(empty), 3, 3, device=dev))
    assert torch.equal(al, c_moment(POLAR, so, d, R, idx_m, n_mol)[0])
    if ds:                                                                       # case f: the scalar head's per-atom charge, then the same reduction
        L = _lib.lib()
        N = s.shape[0]
        qs = torch.full((N, 1), 7.0, device=dev)
        _lib.check(L.spk_atomwise_fwd_f32(fptr(s), fptr(ds[0]), fptr(ds[1]), fptr(ds[2]), fptr(ds[3]), None, N, 128, 64, SILU, n_mol, None, fptr(qs), None, stream()))
        check(tag + " c-abi scalar q", qs, c["ds_q"])
        for name, (correct, with_q) in TO.VARIANTS.items():
            mu, qo = c_moment(DIPOLE, qs, None, R, idx_m, n_mol, total if with_q else None, correct)
            check("%s c-abi scalar mu_%s" % (tag, name), mu, c["ds_mu_" + name])
            check("%s c-abi scalar charges_%s" % (tag, name), qo, c["ds_charges_" + name])


def test_c_abi_without_atoms_and_refusals(dev):
    c, inp, gm, ds, total = case("a", dev)
    so, vo = c_gated(torch.zeros(0, 64, device=dev), torch.zeros(0, 3, 64, device=dev), gm)        # case d: N = 0
    assert so.shape == (0, 1) and vo.shape == (0, 3, 1)
    empty_f, empty_i = torch.zeros(0, device=dev), torch.zeros(0, dtype=torch.long, device=dev)
    mu, _ = c_moment(DIPOLE, empty_f, None, torch.zeros(0, 3, device=dev), empty_i, 2)
    al, _ = c_moment(POLAR, empty_f, empty_f, torch.zeros(0, 3, device=dev), empty_i, 2)
    assert torch.equal(mu, torch.zeros(2, 3, device=dev)) and torch.equal(al, torch.zeros(2, 3, 3, device=dev))
    L = _lib.lib()
    e = TO.case_inputs(GOLD, "e")
    ws = [torch.tensor(np.asarray(w), dtype=torch.float32, device=dev) for w in e["gm"]]
    with pytest.raises(SpkHipError, match="not covered"):                      # case e: no kernel for this head
        c_gated(torch.zeros(4, 64, device=dev), torch.zeros(4, 3, 64, device=dev), ws, n_layers=3)
    assert L.spk_gated_mlp_supported(64, 3, SILU) == 0
    # idx_m that is not ascending: the molecules whose atom range holds a foreign atom come out as NaN, nothing is read out of bounds
    q, R = torch.ones(6, 1, device=dev), torch.ones(6, 3, device=dev)
    mu, _ = c_moment(DIPOLE, q, None, R, torch.tensor([0, 0, 1, 0, 1, 1], device=dev), 2, None, False)
    assert torch.isnan(mu).any()


# ----------------------------------------------------------------------------------------------------------------- operators
@pytest.mark.parametrize("tag", FUSED)
def test_operators(dev, tag):
    c, inp, gm, ds, total = case(tag, dev)
    s, v, R, idx_m, n_mol = inp["scalar_representation"], inp["vector_representation"], inp[properties.R], inp[properties.idx_m], int(c["n_mol"])
    so, vo = torch.ops.spk_hip.gated_mlp(s, v, gm, SILU)
    assert so.shape == (s.shape[0], 1) and vo.shape == (s.shape[0], 3, 1)
    check(tag + " op s_out", so, c["gm_s"])
    check(tag + " op v_out", vo, c["gm_v"])
    so2, vo2 = torch.ops.spk_hip.gated_mlp(s, v, gm, SILU)
    assert torch.equal(so, so2) and torch.equal(vo, vo2)
    # the tile a row falls into does not change its result: the second half of the batch alone
    h = s.shape[0] // 2
    so3, vo3 = torch.ops.spk_hip.gated_mlp(s[h:].clone(), v[h:].clone(), gm, SILU)
    assert torch.equal(so3, so[h:]) and torch.equal(vo3, vo[h:])
    for name, (correct, with_q) in TO.VARIANTS.items():
        mu, q = torch.ops.spk_hip.dipole_moment(so, vo, R, idx_m, n_mol, total if with_q else None, correct)
        assert mu.shape == (n_mol, 3) and q.shape == (s.shape[0], 1)
        check("%s op mu_%s" % (tag, name), mu, c["mu_" + name])
        check("%s op charges_%s" % (tag, name), q, c["charges_" + name])
    al = torch.ops.spk_hip.polarizability(so, vo, R, idx_m, n_mol)
    check(tag + " op alpha", al, c["alpha"])
    assert torch.equal(al, al.transpose(1, 2)) and torch.equal(al, torch.ops.spk_hip.polarizability(so, vo, R, idx_m, n_mol))
    # the oracle fed with the device's own s_out / v_out isolates the reduction
    mu64, _ = TO.dipole(so.cpu().double().numpy(), vo.cpu().double().numpy()[..., 0], c["R"], c["idx_m"], n_mol, c["total_charge"], True)
    check(tag + " op reduction alone", torch.ops.spk_hip.dipole_moment(so, vo, R, idx_m, n_mol, total, True)[0], mu64)


def test_operators_without_atoms_and_refusals(dev):
    c, inp, gm, ds, total = case("a", dev)
    so, vo = torch.ops.spk_hip.gated_mlp(torch.zeros(0, 64, device=dev), torch.zeros(0, 3, 64, device=dev), gm, SILU)
    idx = torch.zeros(0, dtype=torch.long, device=dev)
    mu, q = torch.ops.spk_hip.dipole_moment(so, vo, torch.zeros(0, 3, device=dev), idx, 2, None, True)
    al = torch.ops.spk_hip.polarizability(so, vo, torch.zeros(0, 3, device=dev), idx, 2)
    assert so.shape == (0, 1) and vo.shape == (0, 3, 1) and q.shape == (0, 1)
    assert torch.equal(mu, torch.zeros(2, 3, device=dev)) and torch.equal(al, torch.zeros(2, 3, 3, device=dev))
    e = TO.case_inputs(GOLD, "e")
    ws = [torch.tensor(np.asarray(w), dtype=torch.float32, device=dev) for w in e["gm"]]
    with pytest.raises(RuntimeError, match="no fused kernel"):
        torch.ops.spk_hip.gated_mlp(torch.zeros(4, 64, device=dev), torch.zeros(4, 3, 64, device=dev), ws, SILU)
    with pytest.raises(RuntimeError, match="pyramidal"):                        # right count, wrong widths
        torch.ops.spk_hip.gated_mlp(torch.zeros(4, 64, device=dev), torch.zeros(4, 3, 64, device=dev), gm[:5] + gm[:5], SILU)
    with pytest.raises(RuntimeError, match="float32"):
        torch.ops.spk_hip.gated_mlp(torch.zeros(4, 64, device=dev, dtype=torch.float64), torch.zeros(4, 3, 64, device=dev), gm, SILU)
    # operands that are views at an odd offset are copied, not refused
    big = torch.randn(3 * 64 + 1, device=dev)
    s_off = big[1:].view(3, 64)
    v = inp["vector_representation"]
    a, b = torch.ops.spk_hip.gated_mlp(s_off, v, gm, SILU), torch.ops.spk_hip.gated_mlp(s_off.clone(), v, gm, SILU)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ----------------------------------------------------------------------------------------------------------------- module mirrors
@pytest.mark.parametrize("tag", FUSED + ["e"])
def test_mirrors(dev, tag):
    c, inp, gm, ds, total = case(tag, dev)
    n_mol = int(c["n_mol"])
    with torch.no_grad():
        for name, (correct, with_q) in TO.VARIANTS.items():
            mod = mirror(tag, "dv", dev, return_charges=True, correct_charges=correct)
            assert (mod._gated_act > 0) == (tag != "e")                            # case e has no kernel: the ATen route, and it still matches
            out = mod(batch(inp, total if with_q else None))
            assert out[properties.dipole_moment].shape == (n_mol, 3)
            check("%s mirror mu_%s" % (tag, name), out[properties.dipole_moment], c["mu_" + name])
            check("%s mirror charges_%s" % (tag, name), out[properties.partial_charges], c["charges_" + name])
        out = mirror(tag, "dv", dev, predict_magnitude=True)(batch(inp))
        assert properties.partial_charges not in out and out[properties.dipole_moment].shape == (n_mol,)
        check(tag + " mirror |mu|", out[properties.dipole_moment], c["mag_plain"])
        pol = mirror(tag, "pol", dev)
        al = pol(batch(inp))[properties.polarizability]
        check(tag + " mirror alpha", al, c["alpha"])
        if tag != "e":
            assert torch.equal(al, al.transpose(1, 2)) and torch.equal(al, pol(batch(inp))[properties.polarizability])
            # without a host-side molecule count the module reads idx_m[-1] like the reference (the trailing empty molecule is then not an output)
            short = {k: v for k, v in inp.items() if k != "_n_molecules"}
            assert torch.equal(pol(short)[properties.polarizability], al[:int(c["idx_m"][-1]) + 1])
        if ds:                                                                   # case f
            for name, (correct, with_q) in TO.VARIANTS.items():
                mod = mirror(tag, "ds", dev, return_charges=True, correct_charges=correct)
                assert mod._scalar_act > 0
                out = mod(batch(inp, total if with_q else None))
                check("%s mirror scalar mu_%s" % (tag, name), out[properties.dipole_moment], c["ds_mu_" + name])
                check("%s mirror scalar charges_%s" % (tag, name), out[properties.partial_charges], c["ds_charges_" + name])


def test_mirror_routes(dev):
    """Eval + float32 + device takes the operators (two launches); training mode and float64 take ATen and agree; TorchScript runs the operators."""
    c, inp, gm, ds, total = case("b", dev)
    _lib.profile_enable(True)
    _lib.profile_report()
    mod = mirror("b", "dv", dev, return_charges=True)
    with torch.no_grad():
        want = mod(batch(inp, total))
    torch.cuda.synchronize()
    prof = _lib.profile_report()
    _lib.profile_enable(False)
    assert prof.get("gated_mlp", (0, 0))[0] == 1 and prof.get("moment_reduce", (0, 0))[0] == 1 and set(prof) == {"gated_mlp", "moment_reduce"}, prof
    with torch.no_grad():
        scripted_in = batch(inp, total)
        scripted_in["_n_molecules"] = torch.tensor(int(c["n_mol"]))               # (a scripted module takes tensors only)
        got = torch.jit.script(mod)(scripted_in)
        assert torch.equal(got[properties.dipole_moment], want[properties.dipole_moment]) and torch.equal(got[properties.partial_charges], want[properties.partial_charges])
        train = mod.train()(batch(inp, total))
        check("b mirror train-mode mu_Q", train[properties.dipole_moment], c["mu_Q"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            d64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch(inp, total).items()}
            out64 = mirror("b", "pol", dev).double()(d64)[properties.polarizability]
        assert out64.dtype == torch.float64 and rel(out64, c["alpha"]) < 1e-12
    # training mode carries parameter gradients
    mod.train()
    y = mod(batch(inp, total))[properties.dipole_moment]
    y.square().sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in mod.parameters())


def test_eval_guard_raises_on_backward(dev):
    c, inp, gm, ds, total = case("a", dev)
    for kind, key in (("dv", properties.dipole_moment), ("ds", properties.dipole_moment), ("pol", properties.polarizability)):
        mod = mirror("b", kind, dev) if kind == "ds" else mirror("a", kind, dev)
        d = batch(case("b", dev)[1] if kind == "ds" else inp)
        d["scalar_representation"] = d["scalar_representation"].clone().requires_grad_()
        y = mod(d)[key]
        assert y.requires_grad
        with pytest.raises(RuntimeError, match="eval"):
            y.sum().backward()
        with torch.no_grad():
            assert not mod(d)[key].requires_grad


# ----------------------------------------------------------------------------------------------------------------- fused force call + tail
def _inputs(b, dev):
    inp = M.batch_to_inputs(b, dev)
    n_mol = int(b["n_mol"])
    inp[properties.cell] = (20.0 * torch.eye(3, device=dev)).repeat(n_mol, 1, 1)
    inp[properties.n_atoms] = torch.bincount(b["idx_m"], minlength=n_mol).to(dev)
    return inp


@pytest.mark.parametrize("kind", ["painn", "schnet"])
@pytest.mark.parametrize("mode", [2, 3])
def test_fused_force_call_with_the_heads_behind_it(dev, kind, mode):
    torch.manual_seed(5)
    b = S.molecule_batch("aspirin", 2, seed=11)
    bare = M.build_model(kind)
    rep, head = bare.representation, bare.output_modules[0]
    stress = mode == 3
    tail = ([DipoleMoment(n_in=128, use_vector_representation=True, return_charges=True), Polarizability(n_in=128)] if kind == "painn"
            else [DipoleMoment(n_in=128, return_charges=True)])
    for t in tail:                                  # (the constructor zeroes the biases)
        for name, p in t.named_parameters():
            if name.endswith("bias"):
                torch.nn.init.normal_(p, std=0.2)
    ins = ([Strain()] if stress else []) + [PairwiseDistances()]
    plain = M.NeuralNetworkPotential(rep, input_modules=ins, output_modules=[head, Forces(calc_forces=True, calc_stress=stress)]).to(dev).eval()
    full = M.NeuralNetworkPotential(rep, input_modules=ins, output_modules=[head, Forces(calc_forces=True, calc_stress=stress)] + tail).to(dev).eval()
    assert M.classify_potential(plain) == mode and M.classify_potential(full) == mode and full._n_tail == len(tail)
    want, got = plain(_inputs(b, dev)), full(_inputs(b, dev))
    assert torch.equal(got[properties.energy], want[properties.energy]) and torch.equal(got[properties.forces], want[properties.forces])
    assert set(got) == set(full.model_outputs) and (properties.stress in got) == stress
    # module by module: the same modules, one after the other
    inp = _inputs(b, dev)
    inp[properties.R].requires_grad_()
    for m in list(full.input_modules) + [full.representation] + list(full.output_modules):
        inp = m(inp)
    keys = [properties.dipole_moment, properties.partial_charges] + ([properties.polarizability] if kind == "painn" else [])
    for k in keys:
        check("%s mode %d fused vs modules %s" % (kind, mode, k), got[k], inp[k].detach().cpu().double().numpy())
    # the oracle fed with the device's representation
    fused = full._potential_stress_forward(_inputs(b, dev)) if stress else full._potential_forces_forward(_inputs(b, dev))
    x = fused["scalar_representation"].detach().cpu().double().numpy()
    R, idx_m, n_mol = b["R"].float().double().numpy(), b["idx_m"].numpy(), int(b["n_mol"])
    np64 = lambda ws: [w.detach().cpu().double().numpy() for w in ws]
    if kind == "painn":
        mu_rep = fused["vector_representation"].detach().cpu().double().numpy()
        q, d = TO.gated_mlp(x, mu_rep, np64(tail[0]._head_weights()))
        mu, ch = TO.dipole(q, d[..., 0], R, idx_m, n_mol, None, True)
        a0, da = TO.gated_mlp(x, mu_rep, np64(tail[1]._head_weights()))
        check("%s mode %d alpha vs oracle" % (kind, mode), got[properties.polarizability], TO.polarizability(a0[:, 0], da[..., 0], R, idx_m, n_mol))
        assert torch.equal(got[properties.polarizability], got[properties.polarizability].transpose(1, 2))
    else:
        net = tail[0].outnet
        mu, ch = TO.dipole(TO.mlp(x, np64([net[0].weight, net[0].bias, net[1].weight, net[1].bias])), None, R, idx_m, n_mol, None, True)
    check("%s mode %d mu vs oracle" % (kind, mode), got[properties.dipole_moment], mu)
    check("%s mode %d charges vs oracle" % (kind, mode), got[properties.partial_charges], ch)


# ----------------------------------------------------------------------------------------------------------------- the reference's classes
@pytest.mark.skipif(not refshim.available(), reason="neither the reference sources nor oracle/_ref present")
def test_reference_classes_after_install_give_the_mirrors_outputs(dev):
    """The reference's ``DipoleMoment`` / ``Polarizability`` -- their own ``forward`` -- after ``install()``: the networks inside are the mirror's
    blocks, ``snn.scatter_add`` is the HIP one; on the device they reproduce the mirrors (and the fixture).  The names themselves resolve to the
    mirrors after ``install()``."""
    import schnetpack_amd.install as inst
    from schnetpack_amd import nn as N
    ns = refshim.load()
    ref_dipole, ref_pol = ns.atomwise.DipoleMoment, ns.atomwise.Polarizability
    c, inp, gm, ds, total = case("b", dev)
    maxm = int(c["idx_m"][-1]) + 1
    rd, rp = ref_dipole(n_in=128, use_vector_representation=True, return_charges=True), ref_pol(n_in=128)
    try:
        inst.install(sys.modules["schnetpack"])
        assert sys.modules["schnetpack.atomistic.atomwise"].DipoleMoment is DipoleMoment and sys.modules["schnetpack"].nn.GatedEquivariantBlock is N.GatedEquivariantBlock
        assert ref_dipole is not DipoleMoment and ref_dipole.__module__ == "schnetpack.atomistic.atomwise"
        # (their networks come from the patched builder, as a model built after install() gets them; the classes were instantiated before it
        #  because the reference's Polarizability names itself in super(), and that name now is the mirror)
        build = sys.modules["schnetpack"].nn.build_gated_equivariant_mlp
        assert build is N.build_gated_equivariant_mlp
        rd.outnet, rp.outnet = build(n_in=128, n_out=1), build(n_in=128, n_out=1)
        assert type(rd.outnet[0]) is N.GatedEquivariantBlock and type(rp.outnet[0].mix_vectors) is N.Dense
        sd = {str(k): torch.as_tensor(np.asarray(w), dtype=torch.float32) for k, w in zip(GOLD["b_dv_state_keys"], c["gm"])}
        rd.load_state_dict(sd, strict=True)
        rp.load_state_dict(sd, strict=True)
        rd, rp = rd.to(dev).eval(), rp.to(dev).eval()
        d = batch(inp, total)
        d[properties.n_atoms] = d[properties.n_atoms][:maxm]
        d[properties.total_charge] = total[:maxm]
        with torch.no_grad():
            out_d, out_p = rd(dict(d)), rp(dict(d))
            mine_d = mirror("b", "dv", dev, return_charges=True)(batch(inp, total))
            mine_p = mirror("b", "pol", dev)(batch(inp))
        assert out_d[properties.dipole_moment].shape == (maxm, 3)
        check("reference class mu vs mirror", out_d[properties.dipole_moment], mine_d[properties.dipole_moment][:maxm].cpu().double().numpy())
        check("reference class charges vs mirror", out_d[properties.partial_charges], mine_d[properties.partial_charges].cpu().double().numpy())
        check("reference class alpha vs mirror", out_p[properties.polarizability], mine_p[properties.polarizability][:maxm].cpu().double().numpy())
        check("reference class mu vs fixture", out_d[properties.dipole_moment], c["mu_Q"][:maxm])
        check("reference class alpha vs fixture", out_p[properties.polarizability], c["alpha"][:maxm])
    finally:
        inst.uninstall()
    assert sys.modules["schnetpack.atomistic.atomwise"].DipoleMoment is ref_dipole
