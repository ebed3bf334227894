"""GPU: the SO(3) kernels (csrc/spk_so3.hip) through every route -- the C ABI, the operators ``torch.ops.spk_hip.real_sph_harm`` / ``so3_conv`` /
``so3_product`` with autograd, the module mirrors, SO3net inside the project's and the reference's ``NeuralNetworkPotential`` -- against the numpy
float64 oracle (tests/so3_oracle.py, with the reference's Clebsch-Gordan table from the fixture) and the float64 fixture the reference's own code
produced (tests/golden/so3_cases.npz, tests/make_so3_golden.py).

Tolerance: the project's parity contract, 1e-5 relative in the max-norm, with no extra margin; the reference's own float32
gap on the model cases is below half of it (``gap_*`` in the fixture).  The float64 route on the device is held to the host's 1e-6.  Every test prints
what it measured."""
import copy
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import so3_oracle as SO  # noqa: E402

from schnetpack_amd import _lib, atomistic as A, model as M  # noqa: E402
from schnetpack_amd._lib import fptr, stream  # noqa: E402
from schnetpack_amd.nn import fallback, so3, so3_tables  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1.0e-5
TOL64 = 1.0e-6
G = SO.gold()
rel = SO.rel


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    return torch.device("cuda", 0)


def f32(a, dev, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=dev).requires_grad_(grad)


def as64(t):
    return t.detach().cpu().double().numpy()


# ----------------------------------------------------------------------------------------------------------------- spherical harmonics
def rsh_vectors():
    return np.concatenate([G["rsh_dirs"], np.random.default_rng(8).normal(size=(25, 3))]).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("lmax", SO.LMAXS)
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65])
def test_real_sph_harm_forward_and_gradient(dev, lmax, P):
    S = (lmax + 1) ** 2
    d64 = rsh_vectors()[:P]
    lin = np.random.default_rng(9).normal(size=(max(P, 1), S))[:P]
    d = f32(d64, dev, grad=True).reshape(P, 3)
    Y = torch.ops.spk_hip.real_sph_harm(d, lmax)
    g, = torch.autograd.grad((Y * f32(lin, dev).reshape(P, S)).sum(), d)
    assert Y.shape == (P, S) and g.shape == (P, 3)
    if P == 0:
        return
    lin = as64(f32(lin, dev))
    eY, eg = rel(Y, SO.rsh(d64, lmax)), rel(g, SO.rsh_grad(d64, lmax, lin))
    print("real_sph_harm lmax %d P %d: Y %.2e grad %.2e" % (lmax, P, eY, eg))
    assert eY < TOL and eg < TOL
    if P == 65:      # the fixture's vectors against the reference's own values, and the C ABI
        eF = rel(Y[:40, :], G["rsh_Y"][:, :S])
        Yc = torch.full((P, S), 7.0, device=dev)
        _lib.check(_lib.lib().spk_rsh_fwd_f32(fptr(d.detach()), P, lmax, fptr(Yc), stream()))
        print("real_sph_harm lmax %d: fixture %.2e" % (lmax, eF))
        assert eF < TOL and torch.equal(Yc, Y)


# ----------------------------------------------------------------------------------------------------------------- convolution
_LISTS = {}


def conv_list(kind):
    """(N, idx_i, idx_j, pair vectors) of the cluster batch (1, 2, 5, 70 atoms, every pair of a cluster: rows of 0, 1, 4 and 69 entries) or of the
    4-atom triclinic cell whose cutoff exceeds its edges (repeated (i, j) images, i = j images)."""
    if kind not in _LISTS:
        if kind == "clusters":
            R, _, _, ii, jj = SO.cluster_batch((1, 2, 5, 70), None, 17)
            r = R[jj] - R[ii]
        else:
            R, cell, ii, jj, off = SO.triclinic_cell_case()
            r = R[jj] - R[ii] + off
            key = {(int(a), int(b)) for a, b in zip(ii, jj)}
            assert len(key) < len(ii) and bool((ii == jj).any())                # several images of one (i, j), and self images
        rows = np.bincount(ii, minlength=R.shape[0])
        _LISTS[kind] = (R.shape[0], ii, jj, r, rows)
    return _LISTS[kind]


def conv_inputs(kind, F, lmax, seed=0):
    """float64 arrays holding float32 values.  Y and fcut come from the pair vectors, so the pair (j <- i, -r) sees (-1)^l Y and the same fcut --
    what the plan needs to find the reverse edges."""
    N, ii, jj, r, rows = conv_list(kind)
    rng = np.random.default_rng(100 * F + lmax + seed)
    S, P = (lmax + 1) ** 2, len(ii)
    q = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    d = np.linalg.norm(r, axis=1)
    Y = q(SO.rsh(r / d[:, None], lmax))
    fc = q(0.5 * (np.cos(np.pi * d / (1.05 * d.max())) + 1.0))
    return dict(N=N, ii=ii, jj=jj, x=q(rng.normal(size=(N, S, F))), W=q(rng.normal(size=(P, lmax + 1, F))), Y=Y, fc=fc, gy=q(rng.normal(size=(N, S, F))),
                r=r, rows=rows)


def conv_check(tag, c, lmax, y, gx, gW, gY, gf):
    cg = SO.table(G, lmax)
    ref_y = SO.conv(c["x"], c["W"], c["Y"], c["fc"], c["ii"], c["jj"], cg)
    ref = SO.conv_grads(c["gy"], c["x"], c["W"], c["Y"], c["fc"], c["ii"], c["jj"], cg)
    errs = [rel(y, ref_y)] + [rel(a, b) for a, b in zip((gx, gW, gY, gf), ref)]
    print("so3_conv %-34s y %.2e gx %.2e gW %.2e gY %.2e gfcut %.2e" % ((tag,) + tuple(errs)))
    assert max(errs) < TOL, (tag, errs)
    empty = np.nonzero(c["rows"] == 0)[0]
    assert bool((as64(y)[empty] == 0.0).all())                                   # rows without neighbours: exact zeros


@pytest.mark.parametrize("kind", ["clusters", "cell"])
@pytest.mark.parametrize("lmax", SO.LMAXS)
@pytest.mark.parametrize("F", [32, 64, 160])
def test_so3_conv_operator_forward_and_all_gradients(dev, F, lmax, kind):
    c = conv_inputs(kind, F, lmax)
    ii, jj = torch.tensor(c["ii"], device=dev), torch.tensor(c["jj"], device=dev)
    res = []
    for _ in range(2):
        x, W, Y, fc = f32(c["x"], dev, True), f32(c["W"].reshape(len(c["ii"]), -1), dev, True), f32(c["Y"], dev, True), f32(c["fc"][:, None], dev, True)
        y = torch.ops.spk_hip.so3_conv(x, W, Y, fc, ii, jj, lmax)
        res.append((y.detach(),) + torch.autograd.grad((y * f32(c["gy"], dev)).sum(), [x, W, Y, fc]))
    assert all(torch.equal(a, b) for a, b in zip(*res))                          # no atomics: the same bits on every call
    y, gx, gW, gY, gf = res[0]
    assert gW.shape == (len(c["ii"]), (lmax + 1) * F) and gf.shape == (len(c["ii"]), 1)
    conv_check("%s F %d lmax %d" % (kind, F, lmax), c, lmax, y, gx, gW.reshape(c["W"].shape), gY, gf[:, 0])


@pytest.mark.parametrize("kind", ["clusters", "cell"])
def test_so3_conv_c_abi(dev, kind):
    from schnetpack_amd import ops
    F, lmax = 64, 2
    c = conv_inputs(kind, F, lmax, seed=1)
    L = _lib.lib()
    ii, jj = torch.tensor(c["ii"], device=dev), torch.tensor(c["jj"], device=dev)
    plan = ops.EdgePlan(ii, jj, c["N"], f32(c["r"], dev))
    assert plan.sorted and plan.symmetric
    x, W, Y, fc, gy = (f32(c[k], dev) for k in ("x", "W", "Y", "fc", "gy"))
    y, gx, gW, gY, gf = (torch.full_like(t, 7.0) for t in (x, x, W, Y, fc))
    S = (lmax + 1) ** 2
    _lib.check(L.spk_so3_conv_fwd_f32(fptr(x), fptr(W), fptr(Y), fptr(fc), plan.graph(), lmax, F, fptr(y), stream()))
    ws = torch.empty(int(L.spk_so3_conv_workspace_bytes(plan.graph(), lmax, F)), dtype=torch.uint8, device=dev)
    assert ws.numel() >= len(c["ii"]) * S * 4
    _lib.check(L.spk_so3_conv_bwd_f32(fptr(gy), fptr(x), fptr(W), fptr(Y), fptr(fc), plan.graph(), lmax, F, fptr(gx), fptr(gW), fptr(gY), fptr(gf),
                                      ctypes.c_void_p(ws.data_ptr()), stream()))
    conv_check("C ABI %s F %d lmax %d" % (kind, F, lmax), c, lmax, y, gx, gW, gY, gf)


def small_conv_case(dev, order):
    """SO3Convolution inputs on clusters of 1, 2, 5 and 20 atoms (5 A list), the list as it is, shuffled, or its half (i < j)."""
    R, _, _, ii, jj = SO.cluster_batch((1, 2, 5, 20), 5.0, 7)
    if order == "shuffled":
        p = np.random.default_rng(2).permutation(len(ii))
        ii, jj = ii[p], jj[p]
    elif order == "half":
        keep = ii < jj
        ii, jj = ii[keep], jj[keep]
    r = R[jj] - R[ii]
    d = np.linalg.norm(r, axis=1)
    rng = np.random.default_rng(4)
    q = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    return dict(N=R.shape[0], ii=ii, jj=jj, Y=q(SO.rsh(r / d[:, None], 2)), fc=q(0.5 * (np.cos(np.pi * d / 5.0) + 1.0)), x=q(rng.normal(size=(R.shape[0], 9, 32))),
                rad=q(rng.normal(size=(len(ii), 20))), gy=q(rng.normal(size=(R.shape[0], 9, 32))), rows=np.bincount(ii, minlength=R.shape[0]), r=r)


@pytest.mark.parametrize("order", ["sorted", "shuffled", "half"])
def test_so3_convolution_module_routes_other_lists_to_aten(dev, order):
    c = small_conv_case(dev, order)
    torch.manual_seed(0)
    conv = so3.SO3Convolution(2, 32, 20).to(dev).eval()
    w, b = as64(conv.filternet.weight), as64(conv.filternet.bias)
    c["W"] = (c["rad"] @ w.T + b).reshape(len(c["ii"]), 3, 32)
    x, rad, Y, fc = f32(c["x"], dev, True), f32(c["rad"], dev, True), f32(c["Y"], dev, True), f32(c["fc"][:, None], dev, True)
    n0 = fallback.fallback_count()
    y = conv(x, rad, Y, fc, torch.tensor(c["ii"], device=dev), torch.tensor(c["jj"], device=dev))
    took_aten = fallback.fallback_count() > n0
    gx, grad, gY, gf = torch.autograd.grad((y * f32(c["gy"], dev)).sum(), [x, rad, Y, fc])
    assert took_aten == (order != "sorted"), order
    cg = SO.table(G, 2)
    ref = SO.conv_grads(c["gy"], c["x"], c["W"], c["Y"], c["fc"], c["ii"], c["jj"], cg)
    errs = [rel(y, SO.conv(c["x"], c["W"], c["Y"], c["fc"], c["ii"], c["jj"], cg)), rel(gx, ref[0]), rel(grad, ref[1].reshape(len(c["ii"]), -1) @ w),
            rel(gY, ref[2]), rel(gf, ref[3])]
    print("SO3Convolution %-8s list (%s route): y %.2e gx %.2e gradial %.2e gY %.2e gfcut %.2e" % ((order, "ATen" if took_aten else "kernel") + tuple(errs)))
    assert max(errs) < TOL


# ----------------------------------------------------------------------------------------------------------------- tensor product
@pytest.mark.parametrize("lmax", SO.LMAXS)
@pytest.mark.parametrize("F", [32, 160])
@pytest.mark.parametrize("N", [1, 63, 65])
def test_so3_product_forward_and_gradients(dev, N, F, lmax):
    rng = np.random.default_rng(N + F + lmax)
    S = (lmax + 1) ** 2
    q = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    a, b, gy = (q(rng.normal(size=(N, S, F))) for _ in range(3))
    x1, x2 = f32(a, dev, True), f32(b, dev, True)
    y = torch.ops.spk_hip.so3_product(x1, x2, lmax)
    g1, g2 = torch.autograd.grad((y * f32(gy, dev)).sum(), [x1, x2])
    cg = SO.table(G, lmax)
    r1, r2 = SO.product_grads(gy, a, b, cg)
    errs = [rel(y, SO.product(a, b, cg)), rel(g1, r1), rel(g2, r2)]
    print("so3_product N %d F %d lmax %d: y %.2e gx1 %.2e gx2 %.2e" % ((N, F, lmax) + tuple(errs)))
    assert max(errs) < TOL
    if N == 65 and F == 32:      # the C ABI gives the same bits
        L = _lib.lib()
        yc, c1, c2 = (torch.full_like(y, 7.0) for _ in range(3))
        _lib.check(L.spk_so3_product_fwd_f32(fptr(x1.detach()), fptr(x2.detach()), N, lmax, F, fptr(yc), stream()))
        _lib.check(L.spk_so3_product_bwd_f32(fptr(f32(gy, dev)), fptr(x1.detach()), fptr(x2.detach()), N, lmax, F, fptr(c1), fptr(c2), stream()))
        assert torch.equal(yc, y) and torch.equal(c1, g1) and torch.equal(c2, g2)


@pytest.mark.parametrize("lmax", SO.LMAXS)
def test_compiled_in_table_equals_the_mirror_buffers(dev, lmax):
    L = _lib.lib()
    n = int(L.spk_so3_cg_table(lmax, 0, None, None, None, None))
    mod = so3.SO3TensorProduct(lmax)
    assert n == mod.clebsch_gordan.numel()
    s1, s2, so = ((ctypes.c_int32 * n)() for _ in range(3))
    cv = (ctypes.c_float * n)()
    assert int(L.spk_so3_cg_table(lmax, n, s1, s2, so, cv)) == n
    assert list(s1) == mod.idx_in_1.tolist() and list(s2) == mod.idx_in_2.tolist() and list(so) == mod.idx_out.tolist()
    assert np.array_equal(np.asarray(list(cv), dtype=np.float32), mod.clebsch_gordan.numpy())
    assert int(L.spk_so3_cg_table(4, 0, None, None, None, None)) == -1


# ----------------------------------------------------------------------------------------------------------------- module mirrors
def test_mirror_modules_against_their_aten_route_and_the_fixture(dev):
    # harmonics: kernel (eval) against ATen (train) and the fixture
    d = f32(G["rsh_dirs"], dev)
    rsh = so3.RealSphericalHarmonics(3).to(dev)
    n0 = fallback.fallback_count()
    Yk = rsh.eval()(d)
    assert fallback.fallback_count() == n0
    Ya = rsh.train()(d)
    assert fallback.fallback_count() > n0
    errs = {"Y kernel/ATen": rel(Yk, Ya), "Y kernel/fixture": rel(Yk, G["rsh_Y"])}
    # convolution, product and gates at a kernel width: eval against train
    c = small_conv_case(dev, "sorted")
    torch.manual_seed(1)
    conv, prod, gate, gate0 = (m.to(dev) for m in (so3.SO3Convolution(2, 32, 20), so3.SO3TensorProduct(2), so3.SO3ParametricGatedNonlinearity(32, 2),
                                                  so3.SO3GatedNonlinearity(2)))
    x, rad, Y, fc = f32(c["x"], dev), f32(c["rad"], dev), f32(c["Y"], dev), f32(c["fc"][:, None], dev)
    ii, jj = torch.tensor(c["ii"], device=dev), torch.tensor(c["jj"], device=dev)
    with torch.no_grad():
        n0 = fallback.fallback_count()
        yk, pk, gk = conv.eval()(x, rad, Y, fc, ii, jj), prod.eval()(x, x.flip(0)), gate.eval()(x)
        assert fallback.fallback_count() == n0
        ya, pa, ga = conv.train()(x, rad, Y, fc, ii, jj), prod.train()(x, x.flip(0)), gate.train()(x)
    h = torch.nn.functional.linear(x[:, 0].double().cpu(), gate.scaling.weight.double().cpu(), gate.scaling.bias.double().cpu()).reshape(-1, 3, 32)
    errs.update({"conv kernel/ATen": rel(yk, ya), "product kernel/ATen": rel(pk, pa), "gate eval/train": rel(gk, ga),
                 "gate/formula": rel(gk, x.double().cpu() * torch.sigmoid(h[:, SO.l_of(9)])),
                 "plain gate/formula": rel(gate0(x), x.double().cpu() * torch.sigmoid(x[:, :1].double().cpu()))})
    # the fixture's operator case (F = 4: not a kernel width, the ATen route on the device)
    for l in SO.LMAXS:
        p = "op%d_" % l
        cv = so3.SO3Convolution(l, 4, 5).to(dev).eval()
        with torch.no_grad():
            cv.filternet.weight.copy_(f32(G[p + "fw"], dev))
            cv.filternet.bias.copy_(f32(G[p + "fb"], dev))
            y = cv(f32(G[p + "x"], dev), f32(G[p + "radial"], dev), f32(G[p + "Y"], dev), f32(G[p + "cutoff"], dev), torch.tensor(G[p + "idx_i"], device=dev),
                   torch.tensor(G[p + "idx_j"], device=dev))
            yp = so3.SO3TensorProduct(l).to(dev).eval()(f32(G[p + "x"], dev), f32(G[p + "x2"], dev))
        errs["fixture conv lmax %d" % l], errs["fixture product lmax %d" % l] = rel(y, G[p + "y"]), rel(yp, G[p + "yprod"])
    for k, v in errs.items():
        print("mirror modules: %-24s %.2e" % (k, v))
    assert max(errs.values()) < TOL


# ----------------------------------------------------------------------------------------------------------------- models
@pytest.mark.parametrize("tag", ["M1", "M2", "M3"])
def test_model_cases_through_the_mirror_potential(dev, tag):
    c = SO.model_case(G, tag)
    model = SO.mirror_model(G, tag).to(dev).eval()
    assert M.classify_potential(model) == 0
    n0 = fallback.fallback_count()
    out = SO.run_model(model, SO.model_inputs(c, torch.float32, dev), SO.MODEL_KEYS[tag])
    assert fallback.fallback_count() == n0                                       # every layer on its operator route
    errs = {k: rel(out[k], c[k]) for k in SO.MODEL_KEYS[tag]}
    print("%s float32 device:" % tag, " ".join("%s %.2e" % kv for kv in errs.items()), "| reference's own float32 gap:",
          " ".join("%.2e" % float(c["gap_" + k]) for k in SO.MODEL_KEYS[tag]))
    assert max(errs.values()) < TOL


def test_m1_through_the_reference_potential_after_install(dev):
    from oracle import refshim
    from schnetpack_amd import install
    if not refshim.available():
        pytest.skip("reference (oracle/_ref) not built")
    ns = refshim.load()
    importlib.import_module("schnetpack.nn.so3")
    rnet = importlib.import_module("schnetpack.representation.so3net")
    c = SO.model_case(G, "M1")
    install.install()
    try:
        assert rnet.SO3net.__module__.startswith("schnetpack_amd")
        rep = rnet.SO3net(64, 2, 2, ns.nn.GaussianRBF(20, 7.0), ns.nn.CosineCutoff(7.0))
        model = ns.model.NeuralNetworkPotential(rep, input_modules=[ns.response.Strain(), ns.distances.PairwiseDistances()],
                                                output_modules=[ns.atomwise.Atomwise(64, output_key="energy"), ns.response.Forces(calc_stress=True)])
        model.load_state_dict({k: torch.tensor(v) for k, v in SO.weights(G, "M1").items()}, strict=True)
        model = model.to(dev).eval()
        n0 = fallback.fallback_count()
        out = model(SO.model_inputs(c, torch.float32, dev))
        assert fallback.fallback_count() == n0
    finally:
        install.uninstall()
    errs = {k: rel(out[k], c[k]) for k in SO.MODEL_KEYS["M1"]}
    print("M1 through the reference's NeuralNetworkPotential:", " ".join("%s %.2e" % kv for kv in errs.items()))
    assert max(errs.values()) < TOL


def test_m3_vector_representation_feeds_the_dipole_head(dev):
    c = SO.model_case(G, "M3")
    torch.manual_seed(5)
    head = A.DipoleMoment(32, use_vector_representation=True)
    res = []
    for dtype, where in ((torch.float32, dev), (torch.float64, "cpu")):
        base = SO.mirror_model(G, "M3")
        model = M.NeuralNetworkPotential(base.representation, input_modules=list(base.input_modules), output_modules=[copy.deepcopy(head)])
        model = model.to(where).to(dtype).eval()
        res.append(model(SO.model_inputs(c, dtype, where))["dipole_moment"].detach().cpu().double())
    e = rel(res[0], res[1])
    print("M3 dipole moment from SO3net's vector_representation, device float32 against host float64: %.2e" % e)
    assert res[0].shape == (4, 3) and e < TOL


def test_m2_in_float64_on_the_device(dev):
    c = SO.model_case(G, "M2")
    model = SO.mirror_model(G, "M2").to(dev).double().eval()
    out = SO.run_model(model, SO.model_inputs(c, torch.float64, dev), SO.MODEL_KEYS["M2"])
    errs = {k: rel(out[k], c[k]) for k in SO.MODEL_KEYS["M2"]}
    print("M2 float64 device:", " ".join("%s %.2e" % kv for kv in errs.items()))
    assert max(errs.values()) < TOL64


def test_m2_training_mode_parameter_gradients(dev):
    c = SO.model_case(G, "M2")
    grads = []
    for dtype, where in ((torch.float32, dev), (torch.float64, "cpu")):
        model = SO.mirror_model(G, "M2").to(where).to(dtype).train()
        out = model(SO.model_inputs(c, dtype, where))
        loss = (out["energy"] ** 2).mean() + (out["forces"] ** 2).mean()
        loss.backward()
        params = [p for p in model.parameters() if p.requires_grad]
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
        grads.append(torch.cat([p.grad.reshape(-1).cpu().double() for p in params]))
    e = rel(grads[0], grads[1])
    print("M2 training mode: %d parameter gradients, device float32 against host float64: %.2e" % (grads[0].numel(), e))
    assert e < TOL                                                               # the bar of DESIGN.md section 8 holds for training weight gradients too


def test_second_derivative_through_the_device_route_raises(dev):
    c = SO.model_case(G, "M2")
    model = SO.mirror_model(G, "M2").to(dev).eval()
    inp = SO.model_inputs(c, torch.float32, dev)
    inp["_positions"].requires_grad_()
    x = model.representation(A.PairwiseDistances()(inp))
    E = x["scalar_representation"].pow(2).sum()
    with pytest.raises(RuntimeError, match="training mode"):
        torch.autograd.grad(E, inp["_positions"], create_graph=True)
