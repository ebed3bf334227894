"""Generate the committed fixtures under tests/golden from the LIVE reference
(``/root/reference`` imported through ``oracle/refshim.py``).  TEST INFRASTRUCTURE ONLY.

Run in the build container (the GPU box has no reference):

    python oracle/make_golden.py

Every fixture stores the inputs, the reference outputs and (for seeded-init models) a
checksum of the weights; the weights themselves are reproduced on any box by
``spk_oracle.init_*_params`` (same torch CPU RNG stream as the reference constructors).
The one real-weight fixture (the shipped PaiNN aspirin model,
``interfaces/lammps/examples/aspirin/best_model``) stores its state dict.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim, spk_oracle as O  # noqa: E402
from schnetpack_amd import synthetic as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def ref_inputs(b):
    n_mol = int(b["n_mol"])
    counts = torch.bincount(b["idx_m"], minlength=n_mol)
    return {
        "_atomic_numbers": b["Z"], "_positions": b["R"].clone(), "_idx_i": b["idx_i"],
        "_idx_j": b["idx_j"], "_offsets": b["offsets"], "_idx_m": b["idx_m"],
        "_cell": torch.zeros(n_mol, 3, 3), "_pbc": torch.zeros(3 * n_mol, dtype=torch.bool),
        "_n_atoms": counts,
    }


def checksum(p):
    return float(sum(v.double().abs().sum() for v in p.values()))


def run_reference(ns, rep, head_sd, b):
    aw = ns.atomwise.Atomwise(n_in=rep.n_atom_basis, output_key="energy")
    aw.load_state_dict(head_sd)
    model = ns.model.NeuralNetworkPotential(
        rep, input_modules=[ns.distances.PairwiseDistances()],
        output_modules=[aw, ns.response.Forces()])
    model.eval()
    inp = ref_inputs(b)
    out = model(inp)
    res = {"energy": out["energy"].detach().numpy(), "forces": out["forces"].detach().numpy(),
           "scalar_representation": inp["scalar_representation"].detach().numpy()}
    if "vector_representation" in inp:
        res["vector_representation"] = inp["vector_representation"].detach().numpy()
    return res


def save(name, b, res, **extra):
    arrs = {"in_" + k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in b.items() if k != "cell"}
    arrs.update({"ref_" + k: v for k, v in res.items()})
    arrs.update(extra)
    np.savez_compressed(os.path.join(OUT, name), **arrs)
    print("wrote", name, {k: getattr(v, "shape", v) for k, v in arrs.items()})


def main():
    os.makedirs(OUT, exist_ok=True)
    ns = refshim.load()
    nn = ns.nn

    # --- L0 known answers (the reference's own golden tests, tests/nn/test_radial.py:6-74,
    #     test_cutoff.py:7-42, test_activations.py:7-25, evaluated by the reference modules)
    d = torch.linspace(0.0, 6.0, 25)
    d2 = torch.tensor([[0.0, 0.3], [1.7, 4.99], [5.0, 7.5]])
    ka = {
        "d": d.numpy(), "d2": d2.numpy(),
        "gauss20_5": nn.GaussianRBF(20, 5.0)(d).numpy(),
        "gauss5_1p5_start0p5": nn.GaussianRBF(5, 1.5, start=0.5)(d2).numpy(),
        "bessel20_5": nn.BesselRBF(20, 5.0)(d).numpy(),
        "bessel7_3": nn.BesselRBF(7, 3.0)(d2).numpy(),
        "cos5": nn.CosineCutoff(5.0)(d).numpy(),
        "cos1p8": nn.CosineCutoff(1.8)(d2).numpy(),
        "ssp_x": torch.linspace(-30, 30, 61).numpy(),
        "ssp_y": nn.shifted_softplus(torch.linspace(-30, 30, 61)).numpy(),
    }
    # scatter_add golden incl. trailing dims, dim=1, unsorted indices (nn/scatter.py:7-34)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(17, 3, 8, generator=g)
    idx = torch.randint(0, 6, (17,), generator=g)
    ka["scat_x"] = x.numpy(); ka["scat_idx"] = idx.numpy()
    ka["scat_y0"] = nn.scatter_add(x, idx, dim_size=7).numpy()
    xt = x.permute(1, 0, 2).contiguous()
    ka["scat_y1"] = nn.scatter_add(xt, idx, dim_size=7, dim=1).numpy()
    np.savez_compressed(os.path.join(OUT, "nn_known_answers.npz"), **ka)
    print("wrote nn_known_answers.npz")

    head = O.init_atomwise_params(128, seed=1)

    # --- cfg 1: ethanol, SchNet(128,3), seed 0
    cases = [
        ("schnet_ethanol", "schnet", S.molecule_batch("ethanol", 1, jitter=0.0), dict()),
        ("schnet_aspirin8", "schnet", S.molecule_batch("aspirin", 8, seed=0), dict()),
        ("painn_ethanol", "painn", S.molecule_batch("ethanol", 1, jitter=0.0), dict()),
        ("painn_aspirin8", "painn", S.molecule_batch("aspirin", 8, seed=0), dict()),
        ("schnet_bessel_aspirin2", "schnet", S.molecule_batch("aspirin", 2, seed=3),
         dict(radial="bessel")),
        ("painn_bessel_aspirin2", "painn", S.molecule_batch("aspirin", 2, seed=3),
         dict(radial="bessel")),
        # short cutoff: some pairs beyond the cutoff are kept in the list (skin-style) so that
        # the [d < rc] mask of the cosine cutoff is exercised
        ("schnet_skin_aspirin2", "schnet", S.molecule_batch("aspirin", 2, cutoff=5.0, seed=4),
         dict(cutoff=3.5)),
        ("painn_skin_aspirin2", "painn", S.molecule_batch("aspirin", 2, cutoff=5.0, seed=4),
         dict(cutoff=3.5)),
    ]
    # periodic boundary conditions: 64 water molecules in a 12.4 A box (cell offsets, ~54 neighbours/atom)
    wb = S.water_box(n_side=4, seed=0)
    cases += [("schnet_water192", "schnet", wb, dict()), ("painn_water192", "painn", wb, dict())]
    for name, kind, b, kw in cases:
        cutoff = kw.get("cutoff", 5.0)
        radial = kw.get("radial", "gaussian")
        rb = nn.GaussianRBF(20, cutoff) if radial == "gaussian" else nn.BesselRBF(20, cutoff)
        torch.manual_seed(0)
        if kind == "schnet":
            rep = ns.schnet.SchNet(128, 3, rb, nn.CosineCutoff(cutoff))
            p = O.init_schnet_params(cutoff=cutoff, radial=radial)
        else:
            rep = ns.painn.PaiNN(128, 3, rb, nn.CosineCutoff(cutoff))
            p = O.init_painn_params(cutoff=cutoff, radial=radial)
        sd = rep.state_dict()
        assert all(torch.equal(sd[k], p[k].to(sd[k].dtype)) for k in sd), name
        res = run_reference(ns, rep, head, b)
        save(name + ".npz", b, res, weights_checksum=checksum(p), kind=kind, cutoff=cutoff,
             radial=radial, n_interactions=3)

    # --- real weights: shipped PaiNN aspirin model (2 interactions)
    sys.modules["ase.data"].atomic_masses = np.ones(119)
    m = torch.load(os.path.join(refshim.REF_SRC, "..", "interfaces", "lammps", "examples",
                                "aspirin", "best_model"), map_location="cpu", weights_only=False)
    m.eval()
    rep = m.representation
    head_sd = m.output_modules[0].state_dict()
    b = S.molecule_batch("aspirin", 4, seed=7, jitter=0.03)
    res = run_reference(ns, rep, head_sd, b)
    w = {"w_rep." + k: v.numpy() for k, v in rep.state_dict().items()}
    w.update({"w_head." + k: v.numpy() for k, v in head_sd.items()})
    save("painn_aspirin_pretrained.npz", b, res, kind="painn", cutoff=float(rep.cutoff),
         radial="gaussian", n_interactions=int(rep.n_interactions), **w)


def trained_model_goldens(ns):
    """The reference's five trained rMD17-ethanol PaiNN models (examples/trained_models/rmd17_ethanol/painn_{1..5}/best_model: PaiNN(128, 3,
    20 Gaussians, 5 A) + Atomwise + Forces -- configs[3]'s architecture with TRAINED weights): representation + energy head (no
    postprocessors, like every other fixture) on six jittered ethanol frames.  The weights are not stored (12 MB): the tests load them from
    the same model files (oracle/build_ref.py copies them into oracle/_ref/data) and check them against the checksum stored here."""
    from oracle import build_ref
    sys.modules["ase.data"].atomic_masses = np.ones(119)
    b = S.molecule_batch("ethanol", 6, seed=17, jitter=0.06)
    arrs = {"in_" + k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in b.items() if k != "cell"}
    for k in range(1, 6):
        m = torch.load(build_ref.data_path("rmd17_ethanol_painn_%d.model" % k), map_location="cpu", weights_only=False)
        m.eval()
        rep, head_sd = m.representation, m.output_modules[0].state_dict()
        res = run_reference(ns, rep, head_sd, b)
        for q, v in res.items():
            arrs["ref%d_%s" % (k, q)] = v
        arrs["weights_checksum_%d" % k] = checksum({**rep.state_dict(), **{"head." + kk: v for kk, v in head_sd.items()}})
        w = torch.cat([v.flatten().double() for v in rep.state_dict().values() if v.is_floating_point()])
        arrs["weights_absmax_%d" % k] = float(w.abs().max())
    arrs.update(kind="painn", cutoff=5.0, radial="gaussian", n_interactions=3, n_models=5)
    np.savez_compressed(os.path.join(OUT, "painn_rmd17_ethanol_trained.npz"), **arrs)
    print("wrote painn_rmd17_ethanol_trained.npz", {k: getattr(v, "shape", v) for k, v in arrs.items() if not k.startswith("ref")})


def neighbor_list_goldens(ns):
    """(1) the reference's own precomputed Argon vectors (tests/conftest.py:192-447), lifted out of the
    fixture functions; (2) TorchNeighborList outputs (transform/neighborlist.py:438-553) on seeded
    systems: orthorhombic, triclinic + mixed pbc, a cell smaller than the cutoff (several images of the
    same atom), no pbc, fp64 positions."""
    import ast
    import types
    from oracle import nbl_oracle as NB
    src = open(os.path.join(refshim.REF_SRC, "..", "tests", "conftest.py")).read()
    props = types.SimpleNamespace(Z="_atomic_numbers", R="_positions", cell="_cell", pbc="_pbc", n_atoms="_n_atoms",
                                  idx_i="_idx_i", idx_j="_idx_j", offsets="_offsets", Rij="_Rij")
    env = {"np": np, "torch": torch, "spk": types.SimpleNamespace(properties=props)}
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name in ("environment_periodic", "environment_nonperiodic"):
            node.decorator_list = []
            exec(compile(ast.Module([node], []), "conftest", "exec"), env)
    arrs = {}
    for tag in ("periodic", "nonperiodic"):
        cutoff, p, nb = env["environment_" + tag]()
        arrs[tag + "_cutoff"] = cutoff
        for k in ("_positions", "_cell", "_pbc"):
            arrs[tag + k] = p[k].numpy()
        for k, v in nb.items():
            arrs[tag + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, "nbl_argon.npz"), **arrs)
    print("wrote nbl_argon.npz", {k: getattr(v, "shape", v) for k, v in arrs.items()})

    g = torch.Generator().manual_seed(11)
    cases = {
        "ortho": (torch.rand(60, 3, generator=g) * torch.tensor([7.0, 6.0, 8.0]), torch.diag(torch.tensor([7.0, 6.0, 8.0])), [True, True, True], 5.0),
        "triclinic_mixed": (torch.rand(50, 3, generator=g) * 9.0 - 1.0, torch.tensor([[9.0, 0.0, 0.0], [2.5, 8.0, 0.0], [1.0, -1.5, 10.0]]), [True, True, False], 4.0),
        "small_cell": (torch.rand(12, 3, generator=g) * 3.5, torch.tensor([[3.6, 0.0, 0.0], [0.4, 3.5, 0.0], [0.0, 0.3, 4.0]]), [True, True, True], 5.0),
        "free": (torch.randn(80, 3, generator=g) * 4.0, torch.zeros(3, 3), [False, False, False], 3.0),
        # (positions inside the cell along the periodic axes: TorchNeighborList only searches +-ceil(cutoff/height)
        #  images of the UNWRAPPED positions, so it misses pairs of atoms that sit several cells apart)
        "slab_fp64": (torch.rand(40, 3, generator=g, dtype=torch.float64) * torch.tensor([6.0, 6.5, 12.0], dtype=torch.float64), torch.diag(torch.tensor([6.0, 6.5, 30.0], dtype=torch.float64)), [True, True, False], 4.5),
    }
    arrs = {"names": np.array(sorted(cases))}
    for name, (R, cell, pbc, rc) in cases.items():
        pbc = torch.tensor(pbc)
        nl = ns.neighborlist.TorchNeighborList(rc)
        i, j, off = nl._build_neighbor_list(None, R, cell, pbc, rc)
        S = torch.round(off @ torch.linalg.inv(cell)).long() if bool(pbc.any()) else torch.zeros(i.shape[0], 3, dtype=torch.long)
        order = NB.canonical_order(i, j, S)
        arrs.update({name + "_R": R.numpy(), name + "_cell": cell.numpy(), name + "_pbc": pbc.numpy(), name + "_cutoff": rc,
                     name + "_idx_i": i[order].numpy(), name + "_idx_j": j[order].numpy(), name + "_S": S[order].numpy(),
                     name + "_offsets": off[order].numpy()})
        print("  nbl case", name, "pairs", int(i.shape[0]))
    np.savez_compressed(os.path.join(OUT, "nbl_cases.npz"), **arrs)
    print("wrote nbl_cases.npz")


def ring_polymer_goldens():
    """Execute the reference's own RingPolymer._init_propagator / _main_step (md/integrators.py:152-229)
    and NormalModeTransformer (md/utils/normal_model_transformation.py) on seeded beads.  The two modules
    pull in the whole MD package, so the two methods are lifted out with ``ast`` and run against a
    minimal System stand-in that has exactly the normal-mode properties of md/system.py:444-482."""
    import ast
    import importlib.util
    import types
    md_dir = os.path.join(refshim.REF_SRC, "schnetpack", "md")
    spec = importlib.util.spec_from_file_location("_ref_nmt", os.path.join(md_dir, "utils", "normal_model_transformation.py"))
    nmt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(nmt)
    tree = ast.parse(open(os.path.join(md_dir, "integrators.py")).read())
    rp = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "RingPolymer"][0]
    fns = {}
    env = {"torch": torch, "np": np, "System": object}
    for node in rp.body:
        if isinstance(node, ast.FunctionDef) and node.name in ("_init_propagator", "_main_step"):
            exec(compile(ast.Module([node], []), "integrators", "exec"), env)
            fns[node.name] = env[node.name]

    class Sys:
        def __init__(self, q, p, m, nb):
            self.positions, self.momenta, self.masses = q, p, m
            self.nm_transform = nmt.NormalModeTransformer(nb)
        positions_normal = property(lambda s: s.nm_transform.beads2normal(s.positions),
                                    lambda s, v: setattr(s, "positions", s.nm_transform.normal2beads(v)))
        momenta_normal = property(lambda s: s.nm_transform.beads2normal(s.momenta),
                                  lambda s, v: setattr(s, "momenta", s.nm_transform.normal2beads(v)))

    arrs = {}
    g = torch.Generator().manual_seed(21)
    for nb in (1, 2, 4, 5, 8):
        omega, dt = 40.0 + 3.0 * nb, 0.0005
        me = types.SimpleNamespace(n_beads=nb, omega=omega, time_step=dt)
        omega_normal, prop = fns["_init_propagator"](me)
        me.propagator = prop
        q = torch.randn(nb, 7, 3, generator=g, dtype=torch.float64)
        p = torch.randn(nb, 7, 3, generator=g, dtype=torch.float64)
        m = (torch.rand(1, 7, 1, generator=g, dtype=torch.float64) * 15 + 1)
        sysm = Sys(q.clone(), p.clone(), m, nb)
        fns["_main_step"](me, sysm)
        t = "b%d_" % nb
        arrs.update({t + "omega": omega, t + "dt": dt, t + "C": sysm.nm_transform.c_transform.numpy(),
                     t + "propagator": prop[..., 0, 0].numpy(), t + "omega_normal": omega_normal.numpy(),
                     t + "q": q.numpy(), t + "p": p.numpy(), t + "m": m.numpy(),
                     t + "q_out": sysm.positions.numpy(), t + "p_out": sysm.momenta.numpy()})
    np.savez_compressed(os.path.join(OUT, "md_ring_polymer.npz"), **arrs)
    print("wrote md_ring_polymer.npz", sorted(k for k in arrs if k.startswith("b8_")))


def deploy_goldens(ns):
    """Deployed-model goldens: the shipped PaiNN models processed like
    src/scripts/spkdeploy:16-31 does (dtype casts dropped, AddOffsets.mean -> float32, torch.jit.script), fed
    the input dict interfaces/lammps/pair_schnetpack.cpp:285-301 builds (one system, idx_m = 0, edges in
    neighbour-list order of the LOCAL atom index -- here a random permutation -- and offsets = image shifts).
    Two geometries per model: the free molecule and the same molecule in a small periodic cell (images inside
    the cutoff).  Weights + AddOffsets statistics are stored so that the GPU box can rebuild the model."""
    sys.modules["ase.data"].atomic_masses = np.ones(119)
    casts = ("CastTo64", "CastTo32")
    models = {
        "aspirin": os.path.join(refshim.REF_SRC, "..", "interfaces", "lammps", "examples", "aspirin", "best_model"),
        "ethanol": os.path.join(refshim.REF_SRC, "..", "tests", "testdata", "md_ethanol.model"),
    }
    arrs = {}
    g = torch.Generator().manual_seed(21)
    for name, path in models.items():
        m = torch.load(path, map_location="cpu", weights_only=False)
        if not hasattr(m.representation, "electronic_embeddings"):    # utils/compatibility.py:36-39 (2.0.4 pickles)
            m.representation.electronic_embeddings = []
        m.eval()
        keep = torch.nn.ModuleList()
        for pp in m.postprocessors:                 # spkdeploy:19-29
            if type(pp).__name__ in casts:
                continue
            if type(pp).__name__ == "AddOffsets":
                pp.mean = pp.mean.float()
            keep.append(pp)
        m.postprocessors = keep
        try:
            jm = torch.jit.script(m)
            scripted = True
        except Exception as e:  # pragma: no cover - the eager module computes the same function
            print("  torch.jit.script failed (%s); using the eager module" % type(e).__name__)
            jm, scripted = m, False
        cutoff = float(m.representation.cutoff.item())
        b = S.molecule_batch(name, 1, seed=5, jitter=0.02, cutoff=cutoff)
        Z, R0 = b["Z"], b["R"].float()
        n = int(Z.shape[0])
        cell = torch.tensor([[7.5, 0.0, 0.0], [0.6, 8.0, 0.0], [0.0, -0.4, 7.0]])
        for tag, pbc in (("free", torch.zeros(3, dtype=torch.bool)), ("pbc", torch.ones(3, dtype=torch.bool))):
            R = R0 - R0.min(0).values + 0.3 if tag == "pbc" else R0
            nl = ns.neighborlist.TorchNeighborList(cutoff)
            i, j, off = nl._build_neighbor_list(Z, R, cell if tag == "pbc" else torch.zeros(3, 3), pbc, cutoff)
            perm = torch.randperm(int(i.shape[0]), generator=g)
            i, j, off = i[perm].contiguous(), j[perm].contiguous(), off[perm].float().contiguous()
            inp = {"_positions": R.clone(), "_idx_i": i, "_idx_j": j, "_idx_m": torch.zeros(n, dtype=torch.long), "_offsets": off,
                   "_cell": (cell if tag == "pbc" else torch.zeros(3, 3)), "_n_atoms": torch.tensor([n]), "_atomic_numbers": Z}
            out = jm(inp)
            t = "%s_%s_" % (name, tag)
            arrs.update({t + "Z": Z.numpy(), t + "R": R.numpy(), t + "idx_i": i.numpy(), t + "idx_j": j.numpy(), t + "offsets": off.numpy(),
                         t + "cell": inp["_cell"].numpy(), t + "pbc": pbc.numpy(), t + "energy": out["energy"].detach().float().numpy(),
                         t + "forces": out["forces"].detach().float().numpy()})
            print("  deploy case", t, "edges", int(i.shape[0]), "E", float(out["energy"]), "scripted", scripted)
        rep = m.representation
        arrs[name + "_cutoff"] = cutoff
        arrs[name + "_n_interactions"] = int(rep.n_interactions)
        arrs[name + "_mean"] = float(keep[0].mean) if len(keep) else 0.0
        arrs[name + "_scripted"] = scripted
        if name == "aspirin":       # these weights are already in painn_aspirin_pretrained.npz (w_rep.* / w_head.*)
            arrs[name + "_weights_checksum"] = checksum(rep.state_dict()) + checksum(m.output_modules[0].state_dict())
            continue
        for k, v in rep.state_dict().items():
            arrs[name + "_w_rep." + k] = v.numpy()
        for k, v in m.output_modules[0].state_dict().items():
            arrs[name + "_w_head." + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, "deploy_painn.npz"), **arrs)
    print("wrote deploy_painn.npz")


def deep_model_goldens(ns):
    """The reference's DEFAULT depth (configs/model/representation/schnet.yaml:5-9: n_interactions = 6; PaiNN with six blocks
    beside it): twice the interactions of the bench configuration -- twice the error accumulation of the fp32 kernels (round-2
    review: pin a 6-interaction golden).  Molecule batch and the periodic 192-atom water box."""
    nn = ns.nn
    head = O.init_atomwise_params(128, seed=1)
    wb = S.water_box(n_side=4, seed=0)
    for name, kind, b in (("schnet6_aspirin4", "schnet", S.molecule_batch("aspirin", 4, seed=11)), ("schnet6_water192", "schnet", wb),
                          ("painn6_aspirin4", "painn", S.molecule_batch("aspirin", 4, seed=11)), ("painn6_water192", "painn", wb)):
        rb = nn.GaussianRBF(20, 5.0)
        torch.manual_seed(0)
        if kind == "schnet":
            rep = ns.schnet.SchNet(128, 6, rb, nn.CosineCutoff(5.0))
            p = O.init_schnet_params(n_interactions=6)
        else:
            rep = ns.painn.PaiNN(128, 6, rb, nn.CosineCutoff(5.0))
            p = O.init_painn_params(n_interactions=6)
        sd = rep.state_dict()
        assert all(torch.equal(sd[k], p[k].to(sd[k].dtype)) for k in sd), name
        res = run_reference(ns, rep, head, b)
        save(name + ".npz", b, res, weights_checksum=checksum(p), kind=kind, cutoff=5.0, radial="gaussian", n_interactions=6)


def deep_bessel_goldens(ns):
    """Six interactions x BesselRBF (round-3 review): the molecule kernels evaluate sin / cos with the hardware transcendentals, and
    depth multiplies whatever error they leave -- the least-margin combination gets its own reference fixtures, on a molecule batch
    and on the periodic 192-atom water box."""
    nn = ns.nn
    head = O.init_atomwise_params(128, seed=1)
    wb = S.water_box(n_side=4, seed=0)
    for name, kind, b in (("schnet6_bessel_aspirin4", "schnet", S.molecule_batch("aspirin", 4, seed=11)), ("schnet6_bessel_water192", "schnet", wb),
                          ("painn6_bessel_aspirin4", "painn", S.molecule_batch("aspirin", 4, seed=11)), ("painn6_bessel_water192", "painn", wb)):
        rb = nn.BesselRBF(20, 5.0)
        torch.manual_seed(0)
        if kind == "schnet":
            rep = ns.schnet.SchNet(128, 6, rb, nn.CosineCutoff(5.0))
            p = O.init_schnet_params(n_interactions=6, radial="bessel")
        else:
            rep = ns.painn.PaiNN(128, 6, rb, nn.CosineCutoff(5.0))
            p = O.init_painn_params(n_interactions=6, radial="bessel")
        sd = rep.state_dict()
        assert all(torch.equal(sd[k], p[k].to(sd[k].dtype)) for k in sd), name
        res = run_reference(ns, rep, head, b)
        save(name + ".npz", b, res, weights_checksum=checksum(p), kind=kind, cutoff=5.0, radial="bessel", n_interactions=6)


def collate_goldens(ns):
    """The reference's ``_atoms_collate_fn`` (data/loader.py:13-58) on five seeded systems (tests/test_data_wire.py): the stored
    inputs ``in<s>_<key>`` and the collated batch ``ref_<key>``, so that the collate mirror is checked without the reference."""
    rng = np.random.RandomState(0)
    systems = []
    for kind in ("aspirin", "ethanol", "aspirin", "ethanol", "ethanol"):
        Z, R0 = (S.ASPIRIN_Z, np.asarray(S.ASPIRIN_R)) if kind == "aspirin" else (S.ETHANOL_Z, np.asarray(S.ETHANOL_R))
        R = R0 + 0.05 * rng.randn(*R0.shape)
        ii, jj = S.neighbor_pairs_open(R, 5.0)
        t = torch.arange(min(4, len(ii)))
        systems.append({"_atomic_numbers": torch.tensor(Z), "_positions": torch.from_numpy(R).float(), "_n_atoms": torch.tensor([len(Z)]),
                        "_idx_i": torch.from_numpy(ii), "_idx_j": torch.from_numpy(jj), "_offsets": torch.zeros(len(ii), 3),
                        "_cell": torch.zeros(1, 3, 3), "_pbc": torch.zeros(3, dtype=torch.bool), "energy": torch.from_numpy(rng.randn(1)).float(),
                        "_idx_i_triples": t.clone(), "_idx_j_triples": t.clone(), "_idx_k_triples": t.clone()})
    ref = ns.loader._atoms_collate_fn(systems)
    arrs = {"in%d_%s" % (s, k): v.numpy() for s, d in enumerate(systems) for k, v in d.items()}
    arrs.update({"ref_" + k: v.numpy() for k, v in ref.items()})
    np.savez_compressed(os.path.join(OUT, "collate_reference.npz"), **arrs)
    print("wrote collate_reference.npz", len(arrs), "arrays")


# ------------------------------------------------------------------------------------------------ MD step fixtures
# md_pile / md_verlet / md_simulate / md_fold: the reference's own PILE-L thermostat, velocity-Verlet steps, simulator loop and
# replica folding, lifted method by method with ``ast`` (the modules around them pull in ase / hydra / tqdm) and run against
# small stand-ins that carry exactly the attributes those methods read.  Only arrays and short tags are stored.
#
# The reference's ``units.py`` needs ase, so the lifted code sees a ``spk_units`` stand-in whose kB / fs / hbar are the
# project's KB_MD / FS_MD / HBAR_MD (stored in each fixture that uses them).  The unit constants themselves are therefore
# NOT pinned by these fixtures: ase's CODATA year differs from the project's values in the 7th digit.
MD_FIXTURES = ("md_pile", "md_verlet", "md_simulate", "md_fold")
PILE_BEADS = (1, 2, 3, 4, 5, 8, 16, 32, 64)
# (omega, dt, tau_fs, thermostat_centroid, damping_factor); set 2 is the TRPMD form
PILE_SETS = ((55.0, 5e-4, 100.0, True, 1.0), (157.0, 2e-4, 10.0, True, 1.0), (40.0, 5e-4, 1.0, False, 0.5), (314.0, 5e-4, 1000.0, True, 1.0))
PILE_T, PILE_SEED, PILE_STEP, PILE_WHICH = 300.0, 0x5EED0123456789, 7, 1
# the GPU trajectory test (tests/test_gpu_md_reference.py) bounds positions at 1e-5 and momenta at 1e-4
SIM_TOL_Q, SIM_TOL_P = 1e-5, 1e-4
# time step and time constant (fs; FS_MD makes it 0.4 time units): centroid c1 = exp(-dt / 2 tau) = 0.61, and with the seeded
# SchNet's forces (|F| ~ 0.2 .. 0.8) a kick dt/2 F is ~ 0.1 next to momenta of ~ 0.4 .. 2, so (1 - c1) dt/2 F -- what a swapped
# thermostat / kick pair changes per step -- is percent-level.  At the dt = 0.02 of the NVE tests the orders differ by 4e-4 only.
SIM = dict(n_beads=4, n_steps=6, dt=0.4, omega=3.0, tau_fs=400.0, T=3.0, seed=0xC0FFEE1234)


def _md_path(*parts):
    return os.path.join(refshim.REF_SRC, "schnetpack", "md", *parts)


def _lift(path, cls, names, env):
    """{name: function} of methods ``names`` of class ``cls`` in the reference file ``path``, compiled in memory against ``env``
    (annotations dropped: they name classes of modules that cannot be imported here)."""
    import ast
    tree = ast.parse(open(path).read())
    node = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls][0]
    out = {}
    for fn in node.body:
        if isinstance(fn, ast.FunctionDef) and fn.name in names:
            fn.decorator_list, fn.returns = [], None
            for a in fn.args.args + fn.args.kwonlyargs:
                a.annotation = None
            exec(compile(ast.Module([fn], []), os.path.basename(path), "exec"), env)
            out[fn.name] = env[fn.name]
    missing = set(names) - set(out)
    assert not missing, (path, cls, missing)
    return out


class _TorchWithNoise:
    """``torch`` as the lifted thermostat sees it: ``randn_like`` hands out the prepared noise tensors in order."""

    def __init__(self, noise):
        self._noise = list(noise)

    def randn_like(self, x):
        n = self._noise.pop(0)
        assert n.shape == x.shape
        return n.to(x.dtype)

    def __getattr__(self, name):
        return getattr(torch, name)


def _md_units():
    import types
    from schnetpack_amd import md as MD
    return types.SimpleNamespace(kB=MD.KB_MD, fs=MD.FS_MD, hbar=MD.HBAR_MD)


def _nm_transformer():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_ref_nmt", _md_path("utils", "normal_model_transformation.py"))
    nmt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(nmt)
    return nmt.NormalModeTransformer


class _RingSystem:
    """The attributes of md/system.py that integrators and thermostats touch (normal-mode properties of :444-482)."""

    def __init__(self, q, p, m, n_beads, forces=None):
        self.positions, self.momenta, self.masses, self.n_replicas = q, p, m, n_beads
        self.forces = forces
        self.nm_transform = _nm_transformer()(n_beads).to(p.dtype)       # Simulator.to(precision) casts this buffer
    positions_normal = property(lambda s: s.nm_transform.beads2normal(s.positions),
                                lambda s, v: setattr(s, "positions", s.nm_transform.normal2beads(v)))
    momenta_normal = property(lambda s: s.nm_transform.beads2normal(s.momenta),
                              lambda s, v: setattr(s, "momenta", s.nm_transform.normal2beads(v)))


def _pile_hook_class(noise):
    """The reference's PILELocalThermostat as a plain class: SimulationHook's no-op stages, ThermostatHook's begin / end /
    simulation-start stages and the two PILE-L methods, all lifted."""
    env = {"torch": _TorchWithNoise(noise), "spk_units": _md_units()}
    fns = _lift(_md_path("simulation_hooks", "basic_hooks.py"), "SimulationHook",
                ("on_step_begin", "on_step_middle", "on_step_end", "on_step_finalize", "on_simulation_start", "on_simulation_end"), env)
    fns.update(_lift(_md_path("simulation_hooks", "thermostats.py"), "ThermostatHook", ("on_simulation_start", "on_step_begin", "on_step_end"), env))
    fns.update(_lift(_md_path("simulation_hooks", "thermostats_rpmd.py"), "PILELocalThermostat", ("_init_thermostat", "_apply_thermostat"), env))

    def __init__(self, temperature_bath, time_constant, thermostat_centroid=True, damping_factor=1.0):
        # the buffers of ThermostatHook.__init__ / PILELocalThermostat.__init__: python floats become float32 tensors
        self.temperature_bath = torch.tensor(temperature_bath)
        self.time_constant = torch.tensor(time_constant * env["spk_units"].fs)
        self.thermostat_centroid = torch.tensor(thermostat_centroid)
        self.damping_factor = torch.tensor(damping_factor)
        self.initialized = False
    fns["__init__"] = __init__
    fns["to"] = lambda self, *a: self          # c1 / c2 / thermostat_factor are plain attributes: nn.Module.to leaves them
    return type("LiftedPILELocalThermostat", (), fns)


def _lifted_ring_polymer(n_beads, omega, dt):
    """Namespace with the state of the reference's RingPolymer and its lifted ``_init_propagator`` / ``_main_step`` / ``half_step``."""
    import types
    env = {"torch": torch, "np": np}
    fns = _lift(_md_path("integrators.py"), "RingPolymer", ("_init_propagator", "_main_step"), env)
    fns.update(_lift(_md_path("integrators.py"), "Integrator", ("half_step", "main_step"), env))
    me = types.SimpleNamespace(n_beads=n_beads, omega=omega, time_step=dt)
    me.omega_normal, me.propagator = fns["_init_propagator"](me)
    me._main_step = lambda system: fns["_main_step"](me, system)
    me.main_step = lambda system: fns["main_step"](me, system)
    me.half_step = lambda system: fns["half_step"](me, system)
    return me


def pile_masses_and_momenta(n_beads):
    """7 atoms, masses in [1, 16] with one hydrogen-to-heavy pair (1.008 and 200), thermal-scale momenta (float64)."""
    from schnetpack_amd import md as MD
    g = torch.Generator().manual_seed(100 + n_beads)
    m = torch.rand(1, 7, 1, generator=g, dtype=torch.float64) * 15 + 1
    m[0, 0, 0], m[0, 1, 0] = 1.008, 200.0
    p = torch.randn(n_beads, 7, 3, generator=g, dtype=torch.float64) * (m * MD.KB_MD * n_beads * PILE_T).sqrt()
    return m, p


def md_pile_arrays():
    """tests/golden/md_pile.npz: the lifted ``RingPolymer._init_propagator`` (omega_normal), ``PILELocalThermostat._init_thermostat``
    (c1, c2, thermostat_factor -- float32, the reference's natural dtype: omega_normal is a float32 buffer) and ``_apply_thermostat``
    on seeded momenta with ``torch.randn_like`` returning ``md_oracle.pile_noise(n_beads, 7, seed, step, which)``, once with a
    float32 system (``f32_``) and once with a float64 system (``f64_``; the coefficients stay float32 as in the reference), plus
    the reference's NormalModeTransformer matrix.  Unit constants: the project's (stored), NOT pinned here."""
    import types
    from oracle import md_oracle as MDO
    u = _md_units()
    arrs = {"n_beads": np.array(PILE_BEADS), "sets": np.array([[o, dt, tau, float(c), d] for o, dt, tau, c, d in PILE_SETS]),
            "temperature": PILE_T, "seed": np.uint64(PILE_SEED), "step": PILE_STEP, "which": PILE_WHICH,
            "unit_kB": u.kB, "unit_fs": u.fs, "unit_hbar": u.hbar}
    for nb in PILE_BEADS:
        m, p = pile_masses_and_momenta(nb)
        noise = MDO.pile_noise(nb, 7, PILE_SEED, PILE_STEP, PILE_WHICH)
        arrs.update({"b%d_C" % nb: _nm_transformer()(nb).c_transform.numpy(), "b%d_m" % nb: m.numpy(), "b%d_p" % nb: p.numpy()})
        for s, (omega, dt, tau_fs, centroid, damping) in enumerate(PILE_SETS):
            integ = _lifted_ring_polymer(nb, omega, dt)
            t = "b%d_s%d_" % (nb, s)
            for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
                th = _pile_hook_class([noise])(PILE_T, tau_fs, centroid, damping)
                system = _RingSystem(None, p.to(dtype).clone(), m.to(dtype), nb)
                sim = types.SimpleNamespace(integrator=integ, system=system, device=None, dtype=dtype)
                th.on_simulation_start(sim)
                th.on_step_end(sim)
                if tag == "f32":
                    assert th.c1.dtype == torch.float32 and system.momenta.dtype == torch.float32
                    arrs.update({t + "omega_normal": integ.omega_normal.numpy(), t + "c1": th.c1.reshape(-1).numpy(),
                                 t + "c2": th.c2.reshape(-1).numpy()})
                assert th.thermostat_factor.dtype == dtype
                arrs.update({t + tag + "_thermostat_factor": th.thermostat_factor.numpy(), t + tag + "_p_out": system.momenta.numpy()})
    return arrs


def md_verlet_arrays():
    """tests/golden/md_verlet.npz: the lifted ``Integrator.half_step`` and ``VelocityVerlet._main_step`` (md/integrators.py:59-110)
    on a seeded [3, 11, 3] float64 state: half step, main step, half step."""
    import types
    env = {"torch": torch}
    half = _lift(_md_path("integrators.py"), "Integrator", ("half_step",), env)["half_step"]
    main = _lift(_md_path("integrators.py"), "VelocityVerlet", ("_main_step",), env)["_main_step"]
    g = torch.Generator().manual_seed(31)
    R, p, F = (torch.randn(3, 11, 3, generator=g, dtype=torch.float64) for _ in range(3))
    m = torch.rand(1, 11, 1, generator=g, dtype=torch.float64) * 15 + 1
    me = types.SimpleNamespace(time_step=0.37)
    st = types.SimpleNamespace(positions=R.clone(), momenta=p.clone(), forces=F, masses=m)
    arrs = {"dt": me.time_step, "R": R.numpy(), "p": p.numpy(), "F": F.numpy(), "m": m.numpy()}
    half(me, st)
    arrs["p_half"] = st.momenta.numpy().copy()
    main(me, st)
    arrs["R_main"] = st.positions.numpy().copy()
    half(me, st)
    arrs["p_end"] = st.momenta.numpy().copy()
    return arrs


def sim_setup():
    """The system of the ring-polymer trajectory fixture: 2 aspirin molecules x 4 beads, seeded SchNet weights, the starting
    q0 / p0 of tests/test_gpu_md.py::test_rpmd_loop_conserves_ring_polymer_energy_and_follows_oracle."""
    from oracle import nbl_oracle as NB
    rep_p, head_p = O.init_schnet_params(), O.init_atomwise_params(128, seed=1)
    b = S.molecule_batch("aspirin", 2, seed=2, jitter=0.02)
    N, B = int(b["Z"].shape[0]), SIM["n_beads"]
    masses = torch.where(b["Z"] == 1, 1.008, torch.where(b["Z"] == 6, 12.011, 15.999))
    g = torch.Generator().manual_seed(3)
    q0 = b["R"][None].repeat(B, 1, 1) + 0.03 * torch.randn(B, N, 3, generator=g)
    p0 = 0.2 * torch.randn(B, N, 3, generator=g) * masses[None, :, None].sqrt()

    def forces(q):           # per bead, exact lists, float64
        out = []
        for k in range(B):
            i, j, _, off = NB.batch_neighbor_list(q[k].float(), b["idx_m"], None, None, 5.0)
            bb = dict(b, R=q[k], idx_i=i, idx_j=j, offsets=off.double())
            out.append(O.energy_and_forces("schnet", rep_p, head_p, bb, 3, dtype=torch.float64)["forces"])
        return torch.stack(out)

    return dict(b=b, rep_p=rep_p, head_p=head_p, masses=masses, q0=q0, p0=p0, forces=forces)


def sim_oracle_trajectory(setup, c1, c2, order="reference"):
    """The NVT ring-polymer step of tests/test_gpu_pimd.py:110-116 through ``oracle/md_oracle.py`` (float64) with the thermostat
    coefficients given.  ``order``: "reference" (thermostat, kick, main step, forces, kick, thermostat), or one of the two
    wrong orders the fixture must tell apart: "after_first_kick" (begin-of-step thermostat after the first kick) and
    "before_second_kick" (end-of-step thermostat before the second kick).  Returns q, p after every step."""
    from oracle import md_oracle as MDO
    from schnetpack_amd import md as MD
    B, dt, seed = SIM["n_beads"], SIM["dt"], SIM["seed"]
    N = int(setup["q0"].shape[1])
    C = MDO.normal_mode_matrix(B)
    _, prop = MDO.ring_polymer_propagator(B, SIM["omega"], dt)
    kT = MD.KB_MD * B * SIM["T"]
    q, p, m = setup["q0"].double(), setup["p0"].double(), setup["masses"].double()[None, :, None]
    F = setup["forces"](q)
    qs, ps = [], []
    for step in range(SIM["n_steps"]):
        th = lambda p, which: MDO.pile_apply(p, m, C, c1, c2, kT, MDO.pile_noise(B, N, seed, step, which))
        if order == "after_first_kick":
            p = th(MDO.half_step(p, F, dt), 0)
        else:
            p = MDO.half_step(th(p, 0), F, dt)
        q, p = MDO.ring_polymer_main_step(q, p, m, C, prop)
        F = setup["forces"](q)
        if order == "before_second_kick":
            p = MDO.half_step(th(p, 1), F, dt)
        else:
            p = th(MDO.half_step(p, F, dt), 1)
        qs.append(q)
        ps.append(p)
    return torch.stack(qs), torch.stack(ps)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def md_simulate_arrays():
    """tests/golden/md_simulate.npz: the lifted ``Simulator.simulate`` (md/simulator.py:93-161) for 6 steps with the lifted
    RingPolymer integrator, the lifted PILE-L thermostat and a recording hook (in this order), a float64 system and a calculator
    stand-in that returns ``oracle/spk_oracle.py`` SchNet forces in float64; noise = ``md_oracle.pile_noise(seed, step, which)``.
    Stores q, p after every step, the event order of the first step, the reference's (float32) thermostat coefficients and the
    end states of two WRONG step orders integrated through ``md_oracle`` -- each must be at least 100x the GPU test's tolerance
    away from the reference trajectory, or the fixture could not tell the orders apart.  Unit constants: the project's, NOT pinned."""
    import types
    from contextlib import nullcontext
    from oracle import md_oracle as MDO
    setup = sim_setup()
    B, n_steps, dt = SIM["n_beads"], SIM["n_steps"], SIM["dt"]
    N = int(setup["q0"].shape[1])
    events = []
    noise = [MDO.pile_noise(B, N, SIM["seed"], step, which) for step in range(n_steps) for which in (0, 1)]
    th = _pile_hook_class(noise)(SIM["T"], SIM["tau_fs"])
    lifted_apply = type(th)._apply_thermostat

    def logged_apply(self, simulator):
        events.append("thermostat")
        lifted_apply(self, simulator)
    type(th)._apply_thermostat = logged_apply

    class Recorder:
        def __init__(self, tag):
            self.tag = tag
        def __getattr__(self, name):
            if not name.startswith("on_"):
                raise AttributeError(name)
            return lambda simulator: events.append(name[3:] + " " + self.tag)
    traj_q, traj_p = [], []

    class Snapshot(Recorder):
        def on_step_finalize(self, simulator):
            events.append("step_finalize " + self.tag)
            traj_q.append(simulator.system.positions.clone())
            traj_p.append(simulator.system.momenta.clone())

    integ = _lifted_ring_polymer(B, SIM["omega"], dt)
    half, main = integ.half_step, integ.main_step
    integ.half_step = lambda system: (events.append("half_step"), half(system))[1]
    integ.main_step = lambda system: (events.append("main_step"), main(system))[1]
    system = _RingSystem(setup["q0"].double(), setup["p0"].double(), setup["masses"].double()[None, :, None], B)
    assert system.positions.dtype == torch.float64

    def calculate(sysm):
        events.append("calculate")
        sysm.forces = setup["forces"](sysm.positions)
    sim = types.SimpleNamespace(system=system, integrator=integ, calculator=types.SimpleNamespace(calculate=calculate),
                                simulator_hooks=[th, Snapshot("recorder")], step=0, effective_steps=0, n_steps=None, progress=False,
                                gradients_required=False, device=None, dtype=torch.float64)
    simulate = _lift(_md_path("simulator.py"), "Simulator", ("simulate",), {"torch": torch, "nullcontext": nullcontext, "trange": None})["simulate"]
    simulate(sim, n_steps)
    assert sim.step == n_steps and len(traj_q) == n_steps and not type(th)._apply_thermostat is lifted_apply
    q_ref, p_ref = torch.stack(traj_q), torch.stack(traj_p)
    c1, c2 = th.c1.reshape(-1), th.c2.reshape(-1)
    assert c1.dtype == torch.float32 and float(c1[0]) <= 0.98, c1
    per_step = (len(events) - 3) // n_steps          # initial calculate, simulation_start, ..., simulation_end
    first = events[:2] + events[2:2 + per_step] + events[-1:]
    # sensitivity: the two wrong orders, through the oracle with the SAME coefficients
    arrs = {"n_beads": B, "n_steps": n_steps, "dt": dt, "omega": SIM["omega"], "tau_fs": SIM["tau_fs"], "temperature": SIM["T"],
            "seed": np.uint64(SIM["seed"]), "q0": setup["q0"].numpy(), "p0": setup["p0"].numpy(), "masses": setup["masses"].numpy(),
            "c1": c1.numpy(), "c2": c2.numpy(), "q": q_ref.numpy(), "p": p_ref.numpy(), "events_first_step": np.array(first),
            "weights_checksum": checksum(setup["rep_p"]) + checksum(setup["head_p"]),
            "unit_kB": _md_units().kB, "unit_fs": _md_units().fs, "tol_q": SIM_TOL_Q, "tol_p": SIM_TOL_P}
    for order in ("after_first_kick", "before_second_kick"):
        qw, pw = sim_oracle_trajectory(setup, c1, c2, order)
        dq, dp = _rel(qw[-1], q_ref[-1]), _rel(pw[-1], p_ref[-1])
        print("  wrong order %-18s end state: positions %.3e (tol %.0e), momenta %.3e (tol %.0e)" % (order, dq, SIM_TOL_Q, dp, SIM_TOL_P))
        assert dq >= 100 * SIM_TOL_Q and dp >= 100 * SIM_TOL_P, (order, dq, dp)
        arrs.update({"wrong_%s_q" % order: qw[-1].numpy(), "wrong_%s_p" % order: pw[-1].numpy()})
    return arrs


def fold_system():
    """System stand-in for the replica folding: 2 replicas x (aspirin, ethanol), different cells, mixed pbc."""
    import types
    Z = torch.tensor(S.ASPIRIN_Z + S.ETHANOL_Z)
    R = torch.cat([torch.tensor(S.ASPIRIN_R), torch.tensor(S.ETHANOL_R)]).float()
    n_atoms = torch.tensor([len(S.ASPIRIN_Z), len(S.ETHANOL_Z)])
    cells = torch.tensor([[[12.0, 0.0, 0.0], [1.5, 11.0, 0.0], [0.0, -0.5, 13.0]], [[9.0, 0.0, 0.0], [0.0, 9.5, 0.0], [0.0, 0.0, 30.0]]])
    pbc = torch.tensor([[True, True, True], [True, True, False]])
    return types.SimpleNamespace(n_replicas=2, n_molecules=2, total_n_atoms=int(Z.shape[0]), device=torch.device("cpu"), atom_types=Z,
                                 n_atoms=n_atoms, index_m=torch.repeat_interleave(torch.arange(2), n_atoms),
                                 positions=R[None].repeat(2, 1, 1), cells=cells[None].repeat(2, 1, 1, 1), pbc=pbc[None])


def md_fold_arrays():
    """tests/golden/md_fold.npz: the lifted ``MDCalculator._get_system_molecules`` (md/calculators/base_calculator.py:154-194) on
    ``fold_system()``; the one-replica inputs are stored beside the folded batch."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("_ref_properties", os.path.join(refshim.REF_SRC, "schnetpack", "properties.py"))
    props = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(props)
    fold = _lift(_md_path("calculators", "base_calculator.py"), "MDCalculator", ("_get_system_molecules",), {"torch": torch, "properties": props})
    system = fold_system()
    out = fold["_get_system_molecules"](types.SimpleNamespace(position_conversion=1.0), system)
    arrs = {"in_Z": system.atom_types.numpy(), "in_n_atoms": system.n_atoms.numpy(), "in_idx_m": system.index_m.numpy(),
            "in_positions": system.positions[0].numpy(), "in_cells": system.cells[0].numpy(), "in_pbc": system.pbc[0].numpy(),
            "n_replicas": system.n_replicas}
    names = {props.Z: "Z", props.n_atoms: "n_atoms", props.idx_m: "idx_m", props.R: "positions", props.cell: "cells", props.pbc: "pbc"}
    assert set(out) == set(names)
    arrs.update({names[k]: v.numpy() for k, v in out.items()})
    arrs["keys"] = np.array(sorted(out))
    return arrs


def md_arrays(name):
    return {"md_pile": md_pile_arrays, "md_verlet": md_verlet_arrays, "md_simulate": md_simulate_arrays, "md_fold": md_fold_arrays}[name]()


def save_npz_reproducible(path, arrs):
    """An .npz whose bytes depend on the arrays alone (numpy's own writer stamps every member with the current time)."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrs.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def md_step_goldens(names=MD_FIXTURES):
    for name in names:
        arrs = md_arrays(name)
        path = os.path.join(OUT, name + ".npz")
        save_npz_reproducible(path, arrs)
        print("wrote %s.npz: %d arrays, %d bytes" % (name, len(arrs), os.path.getsize(path)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and all(a in MD_FIXTURES for a in sys.argv[1:]):
        md_step_goldens(sys.argv[1:])
    elif len(sys.argv) > 1 and sys.argv[1] == "collate":
        collate_goldens(refshim.load())
    elif len(sys.argv) > 1 and sys.argv[1] == "deep":
        deep_model_goldens(refshim.load())
    elif len(sys.argv) > 1 and sys.argv[1] == "deep_bessel":
        deep_bessel_goldens(refshim.load())
    elif len(sys.argv) > 1 and sys.argv[1] == "md":
        ring_polymer_goldens()
    elif len(sys.argv) > 1 and sys.argv[1] == "nbl":
        neighbor_list_goldens(refshim.load())
    elif len(sys.argv) > 1 and sys.argv[1] == "deploy":
        deploy_goldens(refshim.load())
    elif len(sys.argv) > 1 and sys.argv[1] == "trained":
        trained_model_goldens(refshim.load())
    else:
        main()
        neighbor_list_goldens(refshim.load())
        ring_polymer_goldens()
        deploy_goldens(refshim.load())
        deep_model_goldens(refshim.load())
        deep_bessel_goldens(refshim.load())
        trained_model_goldens(refshim.load())
        collate_goldens(refshim.load())
        md_step_goldens()
