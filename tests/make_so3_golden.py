"""Generator of tests/golden/so3_cases.npz (a plain script, not collected by pytest):

    python tests/make_so3_golden.py

It runs the reference's own ``nn.so3`` and ``representation.so3net`` (through oracle/refshim.py, imported with ``importlib`` after
``refshim.load()``) and stores ONLY arrays:

  cg<l>_val / _in1 / _in2 / _out / _widx   the reference's sparse real Clebsch-Gordan table and ``SO3Convolution.Widx`` for lmax = 1, 2, 3
  sd_<conv|gate|net>_keys / _shapes        ``state_dict`` keys and shapes of SO3Convolution(2, 64, 20), SO3ParametricGatedNonlinearity(64, 2) and the
                                           SO3net of M2
  rsh_*                                    Y (lmax = 3) at 40 vectors -- unit and not, along the axes, in the coordinate planes -- and the gradient of
                                           a fixed random linear form of Y
  op<l>_*                                  one operator case per lmax: 9 atoms, F = 4, float64: y of SO3Convolution and SO3TensorProduct and the
                                           gradients of a fixed random linear form of y w.r.t. x, radial_ij, dir_ij (Y) and cutoff_ij
  m1_*   the weights of the reference's trained tests/testdata/si16.model (float32; Si16, n_atom_basis 64, 2 interactions, lmax 2, cutoff 7, 20
         Gaussians) in Strain -> PairwiseDistances -> SO3net -> Atomwise -> Forces(calc_stress=True), on a jittered 16-atom diamond cell with the
         all-images list of tests/so3_oracle.py (float64): E, F, stress from a float64 run
  m2_*   seeded SO3net(32, 2, lmax = 3, BesselRBF(20, 5), CosineCutoff(5), shared_interactions=True) + Atomwise + Forces on clusters of 1, 2, 5 and 20
         atoms (an atom with an empty row, rows of one entry): E, F, multipole_representation
  m3_*   the same batch with lmax = 1 and return_vector_representation=True: E, F, multipole_representation, vector_representation
  m<k>_gap_*   max|x32 - x64| / max|x64| of the reference's own float32 run; asserted below half the device tolerance of 1e-5
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim  # noqa: E402
from oracle.make_golden import save_npz_reproducible  # noqa: E402
import so3_oracle as SO  # noqa: E402

OUT = SO.GOLDEN
TOL = 1.0e-5
SI16 = os.path.join(os.path.dirname(refshim.REF_SRC), "tests", "testdata", "si16.model")      # the reference's own trained model file


def reference():
    ns = refshim.load()
    if not hasattr(sys.modules["ase.data"], "atomic_masses"):
        sys.modules["ase.data"].atomic_masses = np.ones(119)
    ns.so3 = importlib.import_module("schnetpack.nn.so3")
    ns.so3net = importlib.import_module("schnetpack.representation.so3net")
    ns.utils = importlib.import_module("schnetpack.utils")
    return ns


def sd_arrays(prefix, sd, out):
    out[prefix + "_keys"] = np.asarray(list(sd.keys()))
    shp = -np.ones((len(sd), 4), dtype=np.int64)
    for k, v in enumerate(sd.values()):
        shp[k, :v.dim()] = list(v.shape)
    out[prefix + "_shapes"] = shp


def rsh_vectors():
    rng = np.random.default_rng(21)
    r = np.sqrt(0.5)
    fixed = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [r, r, 0], [r, 0, -r], [0, -r, r], [2, 0, 3], [0, 1.5, -0.5], [-0.7, 0.2, 0]]
    u = rng.normal(size=(14, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return np.concatenate([np.asarray(fixed, dtype=np.float64), u, rng.normal(size=(14, 3)) * 1.3])


def tables_and_harmonics(ns, out):
    for l in SO.LMAXS:
        c = ns.so3.SO3Convolution(l, 4, 5)
        for k, b in (("val", c.clebsch_gordan), ("in1", c.idx_in_1), ("in2", c.idx_in_2), ("out", c.idx_out), ("widx", c.Widx)):
            out["cg%d_%s" % (l, k)] = b.numpy().copy()
    sd_arrays("sd_conv", ns.so3.SO3Convolution(2, 64, 20).state_dict(), out)
    sd_arrays("sd_gate", ns.so3.SO3ParametricGatedNonlinearity(64, 2).state_dict(), out)
    d = torch.tensor(rsh_vectors(), requires_grad=True)
    lin = torch.tensor(np.random.default_rng(22).normal(size=16))
    Y = ns.so3.RealSphericalHarmonics(3).double()(d)
    g, = torch.autograd.grad((Y * lin).sum(), d)
    out.update(rsh_dirs=d.detach().numpy(), rsh_lin=lin.numpy(), rsh_Y=Y.detach().numpy(), rsh_grad=g.numpy())


def operator_case(ns, l, out):
    rng = np.random.default_rng(30 + l)
    N, F, S, nr = 9, 4, (l + 1) ** 2, 5
    R = SO.cluster(rng, N)
    ii, jj, _ = SO.all_images_list(R, None, 3.6)
    P = len(ii)
    torch.manual_seed(40 + l)
    conv = ns.so3.SO3Convolution(l, F, nr).double()
    with torch.no_grad():
        conv.filternet.bias.normal_()
    prod = ns.so3.SO3TensorProduct(l).double()
    t = lambda a: torch.tensor(a, requires_grad=True)
    x, x2, rad, cut = t(rng.normal(size=(N, S, F))), t(rng.normal(size=(N, S, F))), t(rng.normal(size=(P, nr))), t(rng.uniform(0.2, 1.0, (P, 1)))
    d = R[jj] - R[ii]
    Y = t(ns.so3.RealSphericalHarmonics(l).double()(torch.tensor(d / np.linalg.norm(d, axis=1, keepdims=True))).numpy())
    gy = torch.tensor(rng.normal(size=(N, S, F)))
    y = conv(x, rad, Y, cut, torch.tensor(ii), torch.tensor(jj))
    gx, grad, gY, gcut = torch.autograd.grad((y * gy).sum(), [x, rad, Y, cut])
    yp = prod(x, x2)
    g1, g2 = torch.autograd.grad((yp * gy).sum(), [x, x2])
    p = "op%d_" % l
    out.update({p + "idx_i": ii, p + "idx_j": jj, p + "x": x.detach().numpy(), p + "x2": x2.detach().numpy(), p + "radial": rad.detach().numpy(),
                p + "cutoff": cut.detach().numpy(), p + "Y": Y.detach().numpy(), p + "gy": gy.numpy(), p + "fw": conv.filternet.weight.detach().numpy(),
                p + "fb": conv.filternet.bias.detach().numpy(), p + "y": y.detach().numpy(), p + "gx": gx.numpy(), p + "gradial": grad.numpy(),
                p + "gY": gY.numpy(), p + "gcutoff": gcut.numpy(), p + "yprod": yp.detach().numpy(), p + "gx1": g1.numpy(), p + "gx2": g2.numpy()})


def potential(ns, rep, n_in, stress):
    ins = ([ns.response.Strain()] if stress else []) + [ns.distances.PairwiseDistances()]
    return ns.model.NeuralNetworkPotential(rep, input_modules=ins, output_modules=[ns.atomwise.Atomwise(n_in, output_key="energy"), ns.response.Forces(calc_stress=stress)])


def run(model, arrs, dtype, keys):
    m = model.to(dtype).eval()
    f = lambda a: torch.tensor(a, dtype=dtype)
    n_mol = int(arrs["idx_m"].max()) + 1
    inp = {"_atomic_numbers": torch.tensor(arrs["Z"]), "_positions": f(arrs["R"]), "_cell": f(arrs["cell"]), "_offsets": f(arrs["offsets"]),
           "_idx_i": torch.tensor(arrs["idx_i"]), "_idx_j": torch.tensor(arrs["idx_j"]), "_idx_m": torch.tensor(arrs["idx_m"]),
           "_n_atoms": torch.bincount(torch.tensor(arrs["idx_m"]), minlength=n_mol), "_pbc": torch.zeros(n_mol, 3, dtype=torch.bool)}
    inp = m.initialize_derivatives(inp)
    for mod in m.input_modules:
        inp = mod(inp)
    inp = m.representation(inp)
    for mod in m.output_modules:
        inp = mod(inp)
    return {k: inp[k].detach().double().numpy() for k in keys}


def model_case(tag, model, arrs, keys, out):
    r64 = run(model, arrs, torch.float64, keys)
    model.float()
    sd = model.state_dict()                                                  # float32 weights: what a user's model file holds
    r32 = run(model, arrs, torch.float32, keys)
    p = tag.lower() + "_"
    out.update({p + k: v for k, v in arrs.items()})
    out[p + "wkeys"] = np.asarray(list(sd.keys()))
    for k, v in enumerate(sd.values()):
        out["%sw%d" % (p, k)] = v.detach().numpy().copy()
    for k in keys:
        out[p + k] = r64[k]
        gap = float(np.abs(r32[k] - r64[k]).max() / np.abs(r64[k]).max())
        out[p + "gap_" + k] = np.asarray(gap)
        print("%s %-28s float32 gap %.2e" % (tag, k, gap))
        assert gap < 0.5 * TOL, (tag, k, gap)


def cluster_arrays(sizes, cutoff, seed):
    R, Z, idx_m, ii, jj = SO.cluster_batch(sizes, cutoff, seed)
    return {"R": R, "Z": Z, "idx_m": idx_m, "idx_i": ii, "idx_j": jj, "offsets": np.zeros((len(ii), 3)), "cell": np.zeros((len(sizes), 3, 3))}


def main():
    torch.set_num_threads(1)      # one summation order: the float32 gaps, too, regenerate byte for byte
    torch.use_deterministic_algorithms(True)
    ns = reference()
    out = {}
    tables_and_harmonics(ns, out)
    for l in SO.LMAXS:
        operator_case(ns, l, out)

    # M1: the reference's trained potential
    trained = ns.utils.load_model(SI16, device="cpu").state_dict()
    rep = ns.so3net.SO3net(64, 2, 2, ns.nn.GaussianRBF(20, 7.0), ns.nn.CosineCutoff(7.0))
    m1 = potential(ns, rep, 64, True)
    m1.load_state_dict({k: v for k, v in trained.items() if not k.startswith("postprocessors.")}, strict=True)
    R, cell = SO.si16_cell()
    ii, jj, off = SO.all_images_list(R, cell, 7.0)
    rows = np.bincount(ii, minlength=16)
    print("M1: %d pairs, rows %d..%d, %d self-image pairs, %d parameters" % (len(ii), rows.min(), rows.max(), int((ii == jj).sum()),
                                                                            sum(p.numel() for p in m1.parameters())))
    arrs = {"R": R, "Z": np.full(16, 14, dtype=np.int64), "idx_m": np.zeros(16, dtype=np.int64), "idx_i": ii, "idx_j": jj, "offsets": off, "cell": cell[None]}
    model_case("M1", m1, arrs, ["energy", "forces", "stress"], out)

    # M2 / M3: seeded models on a cluster batch
    batch = cluster_arrays((1, 2, 5, 20), 5.0, 7)
    torch.manual_seed(52)
    m2 = potential(ns, ns.so3net.SO3net(32, 2, 3, ns.nn.BesselRBF(20, 5.0), ns.nn.CosineCutoff(5.0), shared_interactions=True), 32, False)
    sd_arrays("sd_net", m2.representation.state_dict(), out)
    model_case("M2", m2, batch, ["energy", "forces", "multipole_representation"], out)
    torch.manual_seed(53)
    m3 = potential(ns, ns.so3net.SO3net(32, 2, 1, ns.nn.BesselRBF(20, 5.0), ns.nn.CosineCutoff(5.0), shared_interactions=True,
                                        return_vector_representation=True), 32, False)
    model_case("M3", m3, batch, ["energy", "forces", "multipole_representation", "vector_representation"], out)

    save_npz_reproducible(OUT, out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
