"""Point-charge electrostatics, host side (no device): the float64 restatement (tests/electrostatic_oracle.py) and the module mirrors on their
ATen route against the fixture the reference's own code produced (tests/golden/electrostatic_cases.npz, tests/make_electrostatic_golden.py), the
reference's ``state_dict`` layout and k-vectors, the zero-volume error, TorchScript, the classification of models with an electrostatic term, the
link between a charge-predicting head and its consumer, and the names ``install()`` patches."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import electrostatic_oracle as EO  # noqa: E402

from schnetpack_amd import install as I, model as M, properties, torchops  # noqa: E402
from schnetpack_amd import atomistic as A  # noqa: E402
from schnetpack_amd.nn import CosineCutoff, GaussianRBF, SwitchFunction  # noqa: E402
from schnetpack_amd.nn import fallback  # noqa: E402
from schnetpack_amd.representation import PaiNN, SchNet  # noqa: E402

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "electrostatic_cases.npz"))
ORACLE_TOL = 1.0e-10      # two float64 evaluations of the same sums in different orders (up to 3e3 pairs, 3e3 k-vectors)
MIRROR_TOL = 1.0e-10
COULOMB = [(c, v) for c, vs in EO.COULOMB.items() for v in vs]
EWALD = [(c, v) for c, vs in EO.EWALD.items() for v in vs]


def rel(x, ref, scale=None):
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max() if scale is None else scale
    return float(np.abs(np.asarray(x, dtype=np.float64).reshape(ref.shape) - ref).max() / (scale if scale > 0 else 1.0))


def force_scale(case, v):
    """E1, the exact rock-salt lattice: the forces vanish by symmetry, so they are measured against max|E| / a (as the generator does)."""
    return float(np.abs(v["E"]).max() / 5.64) if case == "E1" else None


def inputs_of(c, dtype=torch.float64):
    t = lambda k: torch.tensor(c[k], dtype=dtype if c[k].dtype.kind == "f" else torch.long)
    inp = {properties.R: t("R"), properties.cell: t("cell"), properties.offsets: t("offsets"), properties.idx_i: t("idx_i"),
           properties.idx_j: t("idx_j"), properties.idx_m: t("idx_m"), properties.partial_charges: t("q"), "_n_molecules": torch.tensor(int(c["n_mol"]))}
    inp[properties.R].requires_grad_()
    inp[properties.partial_charges].requires_grad_()
    return inp


def coulomb_mirror(var):
    pot = A.DampedCoulombPotential(SwitchFunction(*EO.SWITCH)) if var.startswith("damped") else A.CoulombPotential()
    return A.EnergyCoulomb("eV", "Ang", pot, "e", use_neighbors_lr=False, cutoff=EO.CUTOFF if var.endswith("_cut") else None)


def ewald_mirror(case, v):
    unit = ("Ha", "Bohr") if case == "E1" else ("eV", "Ang")
    return A.EnergyEwald(float(v["alpha"]), int(v["k_max"]), unit[0], unit[1], "e", use_neighbors_lr=False,
                         screening_fn=SwitchFunction(*EO.SWITCH) if bool(v["screened"]) else None)


def run_module(mod, inp, strain=False):
    if strain:
        inp = A.Strain()(inp)
    inp = A.PairwiseDistances()(inp)
    inp = mod(inp)
    wrt = [inp[properties.R], inp[properties.partial_charges]] + ([inp[properties.strain]] if strain else [])
    g = torch.autograd.grad(inp["e"].sum(), wrt)
    return [inp["e"].detach().numpy(), -g[0].numpy(), g[1].numpy()] + ([g[2].numpy()] if strain else [])


# ----------------------------------------------------------------------------------------------------------------- oracle, fixture
@pytest.mark.parametrize("case,var", COULOMB)
def test_coulomb_restatement_is_pinned_to_the_fixture(case, var):
    c, v = EO.case_inputs(GOLD, case), EO.variant(GOLD, case, var)
    E, F, gq = EO.coulomb_case(c, v)
    assert rel(E, v["E"]) < ORACLE_TOL and rel(F, v["F"]) < ORACLE_TOL and rel(gq, v["dEdq"]) < ORACLE_TOL
    for k in v:
        if k.startswith("gap_"):
            assert float(v[k]) < 0.25e-5, (case, var, k)


@pytest.mark.parametrize("case,var", EWALD)
def test_ewald_restatement_is_pinned_to_the_fixture(case, var):
    c, v = EO.case_inputs(GOLD, case), EO.variant(GOLD, case, var)
    E, F, gq, Er, Ek = EO.ewald_case(c, v)
    assert rel(E, v["E"]) < ORACLE_TOL and rel(F, v["F"], force_scale(case, v)) < ORACLE_TOL and rel(gq, v["dEdq"]) < ORACLE_TOL
    assert rel(Er, v["E_real"]) < ORACLE_TOL and rel(Ek, v["E_rec"]) < ORACLE_TOL
    for k in v:
        if k.startswith("gap_"):
            assert float(v[k]) < 0.25e-5, (case, var, k)


def test_rock_salt_reproduces_the_madelung_constant():
    v = EO.variant(GOLD, "E1", "k4")
    assert float(v["ke"]) == 1.0
    assert abs(-float(v["E"][0]) * 5.64 / 8.0 / EO.MADELUNG_NACL - 1.0) < 1.0e-5


def test_cases_cover_the_kernel_edges():
    c = EO.case_inputs(GOLD, "C1")
    rows = np.bincount(c["idx_i"], minlength=len(c["R"]))
    d = np.linalg.norm(c["R"][c["idx_j"]] - c["R"][c["idx_i"]], axis=1)
    assert 16 in rows and 17 in rows and np.bincount(c["idx_m"]).max() > 64 and (c["q"] == 0).sum() == 1
    assert (d < EO.SWITCH[0]).any() and ((d > EO.SWITCH[0]) & (d < EO.SWITCH[1])).any() and (d > EO.CUTOFF).any()
    c2 = EO.case_inputs(GOLD, "C2")
    assert (c2["idx_i"] < c2["idx_j"]).all() and (np.diff(c2["idx_i"]) < 0).any()
    e3 = EO.case_inputs(GOLD, "E3")
    from schnetpack_amd import _lib
    T, slab = int(_lib.lib().spk_ewald_atom_tile()), int(_lib.lib().spk_ewald_atom_slab())
    counts = np.bincount(e3["idx_m"])
    assert list(counts) == [T - 1, T + 1, 2 * T + 1]
    first = int(counts[:2].sum())
    assert first // slab != (first + counts[2] - 1) // slab          # the largest box spans two slabs
    s = e3["R"][e3["idx_m"] == 2] @ np.linalg.inv(e3["cell"][2])
    assert ((s < 0).any(1) & (s > 1).any(1)).any() and (e3["q"] == 0).sum() == 1
    assert max(abs(e3["q"][e3["idx_m"] == m].sum()) for m in range(3)) > 0.1


# ----------------------------------------------------------------------------------------------------------------- mirrors on the host
@pytest.mark.parametrize("case,var", COULOMB)
def test_coulomb_mirror_on_the_host_in_float64_equals_the_fixture(case, var):
    c, v = EO.case_inputs(GOLD, case), EO.variant(GOLD, case, var)
    mod = coulomb_mirror(var).double()
    n0 = fallback.fallback_count()
    out = run_module(mod, inputs_of(c), strain=case == "C3")
    assert fallback.fallback_count() > n0
    assert rel(out[0], v["E"]) < MIRROR_TOL and rel(out[1], v["F"]) < MIRROR_TOL and rel(out[2], v["dEdq"]) < MIRROR_TOL
    if case == "C3":
        assert rel(out[3], v["W"]) < MIRROR_TOL
    assert rel(float(mod.ke[0]), float(v["ke"])) < 1e-7 and mod._kind == int(v["kind"])
    if var.endswith("_cut"):
        assert rel(float(mod.shift.reshape(-1)[0]), float(v["shift"])) < 1e-12


@pytest.mark.parametrize("case,var", EWALD)
def test_ewald_mirror_on_the_host_in_float64_equals_the_fixture(case, var):
    c, v = EO.case_inputs(GOLD, case), EO.variant(GOLD, case, var)
    mod = ewald_mirror(case, v).double()
    out = run_module(mod, inputs_of(c))
    assert rel(out[0], v["E"]) < MIRROR_TOL and rel(out[1], v["F"], force_scale(case, v)) < MIRROR_TOL and rel(out[2], v["dEdq"]) < MIRROR_TOL


def test_state_dict_layout_and_kvecs_equal_the_reference():
    mods = {"EnergyCoulomb": A.EnergyCoulomb("eV", "Ang", A.DampedCoulombPotential(SwitchFunction(*EO.SWITCH)), "e", cutoff=EO.CUTOFF),
            "EnergyCoulombPlain": A.EnergyCoulomb("eV", "Ang", A.CoulombPotential(), "e", cutoff=EO.CUTOFF),
            "EnergyEwald": A.EnergyEwald(0.16, 2, "eV", "Ang", "e", screening_fn=SwitchFunction(*EO.SWITCH)), "SwitchFunction": SwitchFunction(*EO.SWITCH)}
    for name, m in mods.items():
        sd = m.state_dict()
        assert list(sd.keys()) == [str(k) for k in GOLD["ref/%s/keys" % name]], name
        assert [",".join(str(s) for s in t.shape) for t in sd.values()] == [str(s) for s in GOLD["ref/%s/shapes" % name]], name
    assert tuple(mods["EnergyCoulombPlain"].cutoff.shape) == () and tuple(mods["EnergyCoulombPlain"].shift.shape) == ()
    assert tuple(mods["EnergyCoulomb"].ke.shape) == (1,) and tuple(mods["EnergyEwald"].alpha.shape) == (1,)
    for km in (1, 2, 4):
        kv = A.EnergyEwald(0.16, km, "eV", "Ang", "e").kvecs
        assert kv.dtype == torch.float32 and np.array_equal(kv.double().numpy(), GOLD["ref/kvecs_k%d" % km])
        assert np.array_equal(EO.kvecs(km), GOLD["ref/kvecs_k%d" % km])
    assert A.EnergyEwald(0.16, 4, "eV", "Ang", "e").kvecs.shape == (340, 3)


def test_state_dict_layout_against_the_live_reference():
    from oracle import refshim
    if not refshim.available() or refshim.sourceless():
        pytest.skip("needs the reference sources")
    import make_electrostatic_golden as G
    ns, ref = G.reference_classes()
    SF = ns.nn.SwitchFunction
    pairs = [(ref.EnergyCoulomb("eV", "Ang", ref.DampedCoulombPotential(SF(1.0, 3.0)), "e", cutoff=6.0),
              A.EnergyCoulomb("eV", "Ang", A.DampedCoulombPotential(SwitchFunction(1.0, 3.0)), "e", cutoff=6.0)),
             (ref.EnergyEwald(0.16, 3, "eV", "Ang", "e", screening_fn=SF(1.0, 3.0)), A.EnergyEwald(0.16, 3, "eV", "Ang", "e", screening_fn=SwitchFunction(1.0, 3.0)))]
    for r, m in pairs:
        rs, ms = r.state_dict(), m.state_dict()
        assert list(rs.keys()) == list(ms.keys())
        for k in rs:
            assert rs[k].shape == ms[k].shape and torch.equal(rs[k], ms[k]), k
        m.load_state_dict(rs)


def test_load_state_dict_refreshes_the_host_copies():
    src = A.EnergyCoulomb("kcal/mol", "Ang", A.DampedCoulombPotential(SwitchFunction(2.0, 5.0)), "e", cutoff=8.0)
    dst = A.EnergyCoulomb("eV", "Ang", A.DampedCoulombPotential(SwitchFunction(1.0, 3.0)), "e", cutoff=6.0)
    dst.load_state_dict(src.state_dict())
    assert (dst._on_host, dst._off_host, dst._rc_host) == (2.0, 5.0, 8.0)
    assert dst._ke_host == float(src.ke[0]) and dst._shift_host == float(src.shift.reshape(-1)[0])
    assert dst.coulomb_potential.switch_fn.switch_values() == (2.0, 5.0)
    e = A.EnergyEwald(0.3, 2, "eV", "Ang", "e")
    e.load_state_dict(A.EnergyEwald(0.2, 2, "kcal/mol", "Ang", "e").state_dict())
    assert abs(e._alpha_host - 0.2) < 1e-7


def test_zero_volume_cell_raises_on_the_aten_route():
    c, v = EO.case_inputs(GOLD, "E2"), EO.variant(GOLD, "E2", "k4")
    inp = inputs_of(c)
    inp[properties.cell] = inp[properties.cell].clone()
    inp[properties.cell][0, 2] = inp[properties.cell][0, 1]
    with pytest.raises(A.EnergyEwaldError):
        run_module(ewald_mirror("E2", v).double(), inp)


def test_switch_function_values_and_ends():
    s = SwitchFunction(1.0, 3.0)
    d = torch.tensor([0.5, 1.0, 1.0 + 1e-6, 2.0, 3.0 - 1e-6, 3.0, 4.0], dtype=torch.float64)
    y = s.double()(d)
    assert y[0] == 1 and y[1] == 1 and y[5] == 0 and y[6] == 0 and abs(float(y[3]) - 0.5) < 1e-15 and torch.isfinite(y).all()
    assert torch.allclose(y, EO.switch(d, 1.0, 3.0), atol=1e-15)


def test_filter_short_range():
    c = EO.case_inputs(GOLD, "C1")
    inp = A.PairwiseDistances()(inputs_of(c))
    full = inp[properties.Rij]
    out = A.FilterShortRange(3.0)(inp)
    keep = full.norm(dim=1) <= 3.0
    assert out[properties.Rij_lr] is full and torch.equal(out[properties.idx_i_lr], torch.tensor(c["idx_i"]))
    assert torch.equal(out[properties.Rij], full[keep]) and torch.equal(out[properties.idx_j], torch.tensor(c["idx_j"])[keep])
    assert (properties.idx_i_lr, properties.idx_j_lr, properties.Rij_lr, properties.offsets_lr) == ("_idx_i_lr", "_idx_j_lr", "_Rij_lr", "_offsets_lr")


@pytest.mark.parametrize("which", ["coulomb", "ewald"])
def test_torchscript_of_the_mirrors_on_the_host(which):
    if which == "coulomb":
        c, v = EO.case_inputs(GOLD, "C1"), EO.variant(GOLD, "C1", "damped_cut")
        mod = coulomb_mirror("damped_cut").double()
    else:
        c, v = EO.case_inputs(GOLD, "E2"), EO.variant(GOLD, "E2", "k4_screened")
        mod = ewald_mirror("E2", v).double()
    scripted = torch.jit.script(mod)
    with torch.no_grad():
        inp = A.PairwiseDistances()(inputs_of(c))
        E = scripted({k: (t.detach() if torch.is_tensor(t) else t) for k, t in inp.items()})["e"]
    assert rel(E.numpy(), v["E"]) < MIRROR_TOL


# ----------------------------------------------------------------------------------------------------------------- model level
def _model(kind, outs, ins=None):
    rb, cf = GaussianRBF(20, 5.0), CosineCutoff(5.0)
    rep = SchNet(64, 2, rb, cf) if kind == "schnet" else PaiNN(64, 2, rb, cf)
    return M.NeuralNetworkPotential(rep, input_modules=ins or [A.PairwiseDistances()], output_modules=outs)


@pytest.mark.parametrize("kind", ["schnet", "painn"])
@pytest.mark.parametrize("term", ["coulomb", "ewald"])
def test_models_with_an_electrostatic_term_classify_as_module_by_module(kind, term):
    el = (A.EnergyCoulomb("eV", "Ang", A.CoulombPotential(), "e_el", use_neighbors_lr=False) if term == "coulomb"
          else A.EnergyEwald(0.16, 2, "eV", "Ang", "e_el", use_neighbors_lr=False))
    for outs in ([A.Atomwise(64, output_key="e_nn"), el, A.Aggregation(["e_nn", "e_el"], "energy"), A.Forces()],
                 [el, A.Atomwise(64, output_key="energy"), A.Forces()],
                 [A.Atomwise(64, output_key="energy"), A.Forces(), el]):
        m = _model(kind, outs)
        assert M.classify_potential(m) == 0
        assert not (m._potential or m._potential_forces or m._potential_stress or m._potential_zbl)
    assert M.classify_potential(_model(kind, [A.Atomwise(64, output_key="energy"), A.Forces()])) == 2      # as before


def test_charge_head_is_linked_only_to_a_later_consumer_of_its_key():
    head = lambda **kw: A.DipoleMoment(64, use_vector_representation=True, return_charges=True, **kw)
    el = lambda key="partial_charges": A.EnergyCoulomb("eV", "Ang", A.CoulombPotential(), "e_el", charges_key=key, use_neighbors_lr=False)
    m = _model("painn", [head(), el(), A.Atomwise(64, output_key="e_nn"), A.Aggregation(["e_nn", "e_el"], "energy"), A.Forces()])
    assert m.output_modules[0]._charges_differentiable
    for outs in ([A.Atomwise(64, output_key="energy"), A.Forces(), head()],                     # no consumer: exactly as before
                 [el(), head(), A.Atomwise(64, output_key="energy"), A.Forces()],               # the consumer runs BEFORE the head (charges from the batch)
                 [head(), el("other_charges"), A.Atomwise(64, output_key="energy"), A.Forces()]):
        m = _model("painn", outs)
        assert not any(getattr(o, "_charges_differentiable", False) for o in m.output_modules)
    assert M.classify_potential(_model("painn", [A.Atomwise(64, output_key="energy"), A.Forces(), head()])) == 2


def test_operators_are_registered_and_refuse_host_tensors():
    for name in ("coulomb", "coulomb_backward", "ewald_recip", "ewald_recip_backward"):
        assert name in torchops.OPERATORS and hasattr(torch.ops.spk_hip, name)
    r, q, i, m = torch.zeros(1, 3), torch.zeros(2), torch.zeros(1, dtype=torch.long), torch.zeros(2, dtype=torch.long)
    with pytest.raises(RuntimeError, match="cpu"):
        torch.ops.spk_hip.coulomb(r, q, i, i, m, 1, torch.zeros(8))
    with pytest.raises(RuntimeError, match="cpu"):
        torch.ops.spk_hip.ewald_recip(torch.zeros(2, 3), q, torch.eye(3)[None], m, 1, torch.zeros(26, 3), torch.zeros(2))
    E, Ea, phi = torch.ops.spk_hip.coulomb(r.to("meta"), q.to("meta"), i.to("meta"), i.to("meta"), m.to("meta"), 1, torch.zeros(8, device="meta"))
    assert E.shape == (1,) and Ea.shape == (2,) and phi.shape == (2,)
    E, coef = torch.ops.spk_hip.ewald_recip(torch.zeros(2, 3, device="meta"), q.to("meta"), torch.zeros(1, 3, 3, device="meta"), m.to("meta"), 1,
                                            torch.zeros(26, 3, device="meta"), torch.zeros(2, device="meta"))
    assert E.shape == (1,) and coef.shape == (1, 26, 2)


def test_install_patches_the_six_names_and_uninstall_restores_them():
    names = {"nn": ["SwitchFunction"], "nn.cutoff": ["SwitchFunction"], "atomistic": ["FilterShortRange", "CoulombPotential", "DampedCoulombPotential",
             "EnergyCoulomb", "EnergyEwald"], "atomistic.distances": ["FilterShortRange"],
             "atomistic.electrostatic": ["CoulombPotential", "DampedCoulombPotential", "EnergyCoulomb", "EnergyEwald"]}
    pkg = types.ModuleType("spkstub")
    subs, stubs = {}, {}
    for name, attrs in names.items():
        mod = types.ModuleType("spkstub." + name)
        for a in attrs:
            stubs.setdefault(a, type("Ref" + a, (), {}))
            setattr(mod, a, stubs[a])
        subs[name] = sys.modules["spkstub." + name] = mod
    pkg.nn, pkg.atomistic = subs["nn"], subs["atomistic"]
    mirrors = {"SwitchFunction": SwitchFunction, **{a: getattr(A, a) for a in names["atomistic"]}}
    try:
        log = I.install(pkg)
        for name, attrs in names.items():
            for a in attrs:
                assert "spkstub.%s.%s" % (name, a) in log and getattr(subs[name], a) is mirrors[a], (name, a)
        I.uninstall()
        for name, attrs in names.items():
            for a in attrs:
                assert getattr(subs[name], a) is stubs[a], (name, a)
    finally:
        I.uninstall()
        for name in subs:
            sys.modules.pop("spkstub." + name, None)
