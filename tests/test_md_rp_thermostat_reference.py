"""CPU: the ring-polymer thermostats beyond PILE-L (NHC on the normal modes, PILE-G, TRPMD; md/simulation_hooks/thermostats_rpmd.py
of the reference) against tests/golden/md_rp_thermostat.npz, which tests/make_md_rp_thermostat_golden.py produces by executing the
reference's OWN lifted methods.  Pinned here: tests/md_rp_thermostat_oracle.py (the float64 restatement the GPU tests compare
with: 1e-12 against the fixture), the host constants of the new classes of ``schnetpack_amd.md`` (frequencies, thermostat masses,
degrees of freedom, PILE-G matrices) and the argument checks of the new entry points of the built library.

The fixture's float64 runs carry the reference's float32-rounded buffers (time constant, frequency, kT, omega_normal); they are
stored and handed to the oracle, so 1e-12 holds.  Unit constants are not pinned.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import load_npz, rel_err
from oracle import md_oracle as MDO

import md_rp_thermostat_oracle as RO

APPS = (1, 2, 6)
STATE_AT = (1, 6)
NHC_CASES = ("b1_l3_m2_o3", "b3_l2_m4_o5", "b4_l1_m1_o3")


@pytest.fixture(scope="module")
def g():
    return load_npz("md_rp_thermostat.npz")


def T(x):
    return torch.from_numpy(np.asarray(x))


def layout(g):
    return T(g["idx_m"]), T(g["n_atoms"])


def test_fixture_holds_the_stated_cases(g):
    assert list(g["n_atoms"]) == [2, 5, 9] and tuple(g["applications"]) == APPS and tuple(g["state_at"]) == STATE_AT
    assert tuple(g["nhc_cases"]) == NHC_CASES
    params = {t: tuple(int(x) for x in r) for t, r in zip(g["nhc_cases"], g["nhc_params"])}
    assert sorted({p[0] for p in params.values()}) == [1, 3, 4]                  # bead counts
    assert len({p[1:] for p in params.values()}) == 3 and any(p[1] == 1 for p in params.values())   # three chain set-ups, one of length 1
    gaps = g["nhc_gaps"]
    assert gaps.shape == (3, 2, 3, 3)                     # case, local / global, p / v / f, application
    for tag in NHC_CASES:
        B, L = params[tag][:2]
        for local in (True, False):
            for k in APPS:
                ref, gap = RO.fixture_nhc(g, tag, local, "p", k)
                assert ref.shape == (B, 16, 3) and ref.dtype == torch.float64 and 0 < gap < 1e-3 * float(ref.abs().max())
            for k in STATE_AT:
                for key in "vf":
                    ref, gap = RO.fixture_nhc(g, tag, local, key, k)
                    assert ref.shape == (B, 16, 3, L) and gap > 0
    assert np.isnan(gaps[:, :, 1:, 1]).all()                 # no chain state after 2 applications
    assert tuple(g["pile_beads"]) == (1, 3, 4) and tuple(g["trpmd_beads"]) == (3, 4)
    assert [str(c) for c in g["pile_cases"]] == ["pg_b1", "pg_b3", "pg_b4", "pgs", "tr_b3", "tr_b4"] and bool((g["pile_gaps"][1:] > 0).all())
    assert g["p_b3"].shape == (3, 16, 3) and int(g["pgs_n_beads"]) == 3
    # a few tens of kilobytes: float64 results only, nothing stored twice (the generator's docstring says how)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "md_rp_thermostat.npz")) < 80 * 1024


@pytest.mark.parametrize("local", [True, False])
@pytest.mark.parametrize("tag", NHC_CASES)
def test_oracle_nhc_rp_matches_the_reference(g, tag, local):
    B, L, ms, order = (int(x) for x in g["nhc_params"][list(g["nhc_cases"]).index(tag)])
    name = "nhc_%s_%s" % (tag, "loc" if local else "glo")
    idx_m, n = layout(g)
    p, m = T(g["p_b%d" % B]).clone(), T(g["m_b%d" % B]).reshape(-1)
    C = MDO.normal_mode_matrix(B)
    (kT, frequency, _), steps = (float(x) for x in g["nhc_%s_consts" % tag]), T(g["nhc_%s_steps" % tag])
    w = RO.rp_nhc_frequencies(T(g["nhc_%s_omega_normal" % tag]).double(), frequency)
    masses = RO.rp_nhc_masses(kT, w, RO.rp_nhc_dof(B, idx_m, n, local), L)
    assert rel_err(masses[:, :, 0, :], T(g[name + "_masses"])) < 1e-12
    v, f = torch.zeros(B, 16, 3, L, dtype=torch.float64), torch.zeros(B, 16, 3, L, dtype=torch.float64)
    for k in range(1, 7):
        p = RO.rp_nhc_apply(p, m, idx_m, n, C, kT, masses, v, f, steps, ms, local)
        if k in APPS:
            assert rel_err(p, RO.fixture_nhc(g, tag, local, "p", k)[0]) < 1e-12, k
        if k in STATE_AT:
            assert rel_err(v, RO.fixture_nhc(g, tag, local, "v", k)[0]) < 1e-12 and rel_err(f, RO.fixture_nhc(g, tag, local, "f", k)[0]) < 1e-12, k
    # the thermostat does something, and the float32 run of the reference is close but not equal
    assert rel_err(p, T(g["p_b%d" % B])) > 1e-3
    ref, gap = RO.fixture_nhc(g, tag, local, "p", 6)
    assert 0 < gap < 1e-4 * float(ref.abs().max())


def noise(g, B, N=16):
    return [MDO.pile_noise(B, N, int(g["seed"]), step, 0) for step in range(6)]


@pytest.mark.parametrize("B", [1, 3, 4])
def test_oracle_pile_global_on_a_batch_is_the_reference_per_molecule(g, B):
    idx_m, n = layout(g)
    p, m = T(g["p_b%d" % B]).clone(), T(g["m_b%d" % B]).reshape(-1)
    C, (c1, c2) = MDO.normal_mode_matrix(B), T(g["pg_b%d_c12" % B])
    kT = float(g["unit_kB"]) * B * float(g["temperature_bath"])
    xi = noise(g, B)
    for k in range(1, 7):
        p, alpha = RO.pile_global_apply(p, m, idx_m, n, C, c1, c2, kT, xi[k - 1])
        if k in APPS:
            assert rel_err(p, RO.fixture_pile(g, "pg_b%d" % B, k)) < 1e-12, k
    assert alpha.shape == (3,) and len({round(float(a), 6) for a in alpha}) == 3          # every molecule its own factor


def test_oracle_pile_global_single_molecule_is_the_reference_unsliced(g):
    B = int(g["pgs_n_beads"])
    idx_m, n = torch.zeros(16, dtype=torch.long), torch.tensor([16])
    p, m = T(g["p_b%d" % B]).clone(), T(g["m_b%d" % B]).reshape(-1)
    c1, c2 = T(g["pgs_c12"])
    kT = float(g["unit_kB"]) * B * float(g["temperature_bath"])
    xi = noise(g, B)
    for k in range(1, 7):
        p, _ = RO.pile_global_apply(p, m, idx_m, n, MDO.normal_mode_matrix(B), c1, c2, kT, xi[k - 1])
        if k in APPS:
            assert rel_err(p, RO.fixture_pile(g, "pgs", k)) < 1e-12, k


@pytest.mark.parametrize("B", [3, 4])
def test_oracle_trpmd_is_pile_without_centroid_and_with_damping(g, B):
    p, m = T(g["p_b%d" % B]).clone(), T(g["m_b%d" % B]).reshape(1, -1, 1)
    c1, c2 = T(g["tr_b%d_c12" % B])
    assert float(c1[0]) == 1.0 and float(c2[0]) == 0.0            # centroid untouched
    kT = float(g["unit_kB"]) * B * float(g["temperature_bath"])
    xi = noise(g, B)
    for k in range(1, 7):
        p = MDO.pile_apply(p, m, MDO.normal_mode_matrix(B), c1, c2, kT, xi[k - 1])
        if k in APPS:
            assert rel_err(p, RO.fixture_pile(g, "tr_b%d" % B, k)) < 1e-12, k


def test_oracle_pile_global_alpha_of_a_molecule_at_rest_or_without_atoms_is_one():
    """A self-check of the ORACLE (no product code runs here): its restatement of the two decisions for K = 0 and for a molecule
    without atoms -- alpha = 1, nothing non-finite, centroid untouched -- which the reference does not make (it divides by zero), so
    no fixture can pin them.  ``k_pile_alpha`` is held to the same decisions by the GPU tests, which compare with this oracle."""
    n = torch.tensor([0, 2, 0])
    idx_m = torch.tensor([1, 1])
    p = torch.zeros(3, 2, 3, dtype=torch.float64)             # the first application of every run: momenta zero
    C = MDO.normal_mode_matrix(3)
    c1, c2 = torch.tensor([0.9, 0.5, 0.5]), torch.tensor([0.1, 0.8, 0.8])
    out, alpha = RO.pile_global_apply(p, torch.ones(2, dtype=torch.float64), idx_m, n, C, c1.double(), c2.double(), 2.5, MDO.pile_noise(3, 2, 1, 0, 0))
    assert alpha.tolist() == [1.0, 1.0, 1.0] and bool(torch.isfinite(out).all())
    assert float(out.sum(0).abs().max()) < 1e-12


# ----------------------------------------------------------------------------- host constants of the classes
@pytest.mark.parametrize("local", [True, False])
@pytest.mark.parametrize("tag", NHC_CASES)
def test_nhc_rp_class_constants(g, tag, local):
    from schnetpack_amd import md as MD
    B, L, ms, order = (int(x) for x in g["nhc_params"][list(g["nhc_cases"]).index(tag)])
    name = "nhc_%s_%s" % (tag, "loc" if local else "glo")
    idx_m, n = layout(g)
    rp = MD.RingPolymer(float(g["dt"]), B, float(g["temperature_bath"]))
    A_before = rp.A.clone()
    th = MD.NHCRingPolymerThermostat(float(g["temperature_bath"]), float(g["tau_fs"]), local=local, chain_length=L, multi_step=ms,
                                     integration_order=order).init(rp, idx_m, n)
    assert torch.equal(rp.A, A_before)                      # the propagator of the integrator is left alone
    # the reference's constants are float32-rounded (time constant, kT: 2^-24 each, squared frequency twice)
    assert rel_err(th.masses[:, :, 0, :], T(g[name + "_masses"])) < 6 * 2.0 ** -24
    assert torch.equal(th.degrees_of_freedom, RO.rp_nhc_dof(B, idx_m, n, local))
    assert rel_err(torch.tensor(th.sub_steps, dtype=torch.float64), T(g["nhc_%s_steps" % tag])) < 2.0 ** -23
    assert abs(th.kb_temperature - float(g["nhc_%s_consts" % tag][0])) < 2.0 ** -22 * th.kb_temperature
    # without a layout the atom count is unknown until the first prepare / application: a clear error, no AttributeError
    bare = MD.NHCRingPolymerThermostat(float(g["temperature_bath"]), float(g["tau_fs"]), local=local, chain_length=L).init(rp)
    for prop in ("masses", "degrees_of_freedom"):
        with pytest.raises(RuntimeError, match="number of atoms is not known"):
            getattr(bare, prop)
    assert float(th.frequencies[0]) == 0.5 / th.time_constant
    with pytest.raises(ValueError):
        MD.NHCRingPolymerThermostat(300.0, 10.0, integration_order=4)
    with pytest.raises(ValueError):
        MD.NHCRingPolymerThermostat(300.0, 10.0, chain_length=0)


@pytest.mark.parametrize("B", [1, 3, 4])
def test_pile_global_and_trpmd_class_constants(g, B):
    from schnetpack_amd import md as MD
    rp = MD.RingPolymer(float(g["dt"]), B, float(g["temperature_bath"]))
    th = MD.PILEGlobalThermostat(float(g["temperature_bath"]), float(g["tau_fs"]), seed=3).init(rp, *layout(g))
    loc = MD.PILELocalThermostat(float(g["temperature_bath"]), float(g["tau_fs"]), seed=3).init(rp)
    C = MD.normal_mode_matrix(B)
    c1, c2 = MD.pile_coefficients(B, rp.omega, rp.time_step, th.time_constant)
    assert th.c1_centroid == float(c1[0]) and abs(th.c1_centroid - float(g["pg_b%d_c12" % B][0, 0])) < 2.0 ** -22
    # M of PILE-L minus the centroid: M1 = M1_L - c1[0] C0^T C0, M2 = M2_L with column 0 zero
    M1 = loc.M[0].double() - c1[0] * torch.outer(C[0], C[0])
    assert float((th.M[0].double() - M1).abs().max()) < 2.0 ** -22
    assert float(th.M[1][:, 0].abs().max()) == 0.0 and torch.equal(th.M[1][:, 1:], loc.M[1][:, 1:])
    assert th.noise_scale == loc.noise_scale and th.ring_polymer
    tr = MD.TRPMDThermostat(float(g["temperature_bath"]), 0.5, seed=3).init(rp)
    par = MD.PILELocalThermostat(float(g["temperature_bath"]), 1.0, thermostat_centroid=False, damping_factor=0.5, seed=3).init(rp)
    assert torch.equal(tr.M, par.M) and tr.noise_scale == par.noise_scale and tr.seed == par.seed
    assert isinstance(tr, MD.PILELocalThermostat) and isinstance(th, MD.PILELocalThermostat)


def test_rpmd_simulation_refuses_what_is_not_a_ring_polymer_thermostat():
    from schnetpack_amd import md as MD
    sim = MD.RPMDSimulation.__new__(MD.RPMDSimulation)
    sim.thermostat, sim.n_beads, sim.n_local, sim._n1 = MD.NHCThermostat(300.0, 10.0), 2, 2, 3
    sim.group, sim.exchange, sim._dist, sim._world, sim._lo = None, "state", False, 1, 0
    sim._rp = MD.RingPolymer(5e-4, 2, 300.0)
    sim._idx_m1, sim._n_atoms1 = torch.zeros(3, dtype=torch.long), torch.tensor([3])
    with pytest.raises(ValueError, match="ring-polymer thermostat"):
        sim._setup_state(torch.zeros(6, 3), torch.ones(3))


# ----------------------------------------------------------------------------- the built library
ENTRIES = ("spk_md_rp_centroid_f32", "spk_md_rp_nhc_f32", "spk_md_pile_alpha_f32", "spk_md_pile_global_f32")


def test_header_declares_the_ring_polymer_thermostat_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "spk_hip.h")).read()
    for name in ENTRIES:
        assert "int %s(" % name in text, name


def test_library_has_the_entries_and_refuses_bad_arguments():
    from schnetpack_amd._lib import SpkHipError, check, lib
    L = lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
    X = ctypes.c_void_p(0x1000)          # a non-null address the checks compare and never follow
    Y = ctypes.c_void_p(0x2000)
    steps = (ctypes.c_float * 7)(*([1e-4] * 7))

    def nhc(p_all=X, masses=X, C=X, lm=X, B=4, N=5, bead0=0, n_local=4, chain=3, ms=2, order=3, sub=steps, kT=1.0, vel=X, frc=X, out=Y):
        return L.spk_md_rp_nhc_f32(p_all, masses, C, lm, B, N, bead0, n_local, chain, ms, order, sub, kT, vel, frc, None, None, 0, None, out, None)

    def pile(p_all=X, masses=X, M=X, B=4, N=5, bead0=0, n_local=4, p_c=X, alpha=X, idx_m=X, out=Y):
        return L.spk_md_pile_global_f32(p_all, masses, M, 1.0, 0, 0, None, 0, B, N, bead0, n_local, p_c, alpha, idx_m, 1, None, out, None)

    bad = [("n_beads", lambda: nhc(B=0)), ("n_beads", lambda: nhc(B=65)), ("bead range", lambda: nhc(bead0=2, n_local=3)),
           ("bead range", lambda: nhc(bead0=-1)), ("bead range", lambda: nhc(bead0=4, n_local=1)), ("alias", lambda: nhc(out=X)),
           ("chain_length", lambda: nhc(chain=0)), ("chain_length", lambda: nhc(chain=17)), ("integration_order", lambda: nhc(order=4)),
           ("multi_step", lambda: nhc(ms=0)), ("sub-step", lambda: nhc(sub=None)), ("null", lambda: nhc(p_all=None)), ("null", lambda: nhc(masses=None)),
           ("null", lambda: nhc(C=None)), ("null", lambda: nhc(lm=None)), ("null", lambda: nhc(vel=None)), ("null", lambda: nhc(frc=None)),
           ("null", lambda: nhc(out=None)), ("idx_m", lambda: L.spk_md_rp_nhc_f32(X, X, X, X, 4, 5, 0, 4, 3, 2, 3, steps, 1.0, X, X, X, None, 1, None, Y, None)),
           ("n_beads", lambda: pile(B=0)), ("n_beads", lambda: pile(B=65)), ("bead range", lambda: pile(bead0=3, n_local=2)), ("alias", lambda: pile(out=X)),
           ("null", lambda: pile(p_all=None)), ("null", lambda: pile(p_c=None)), ("null", lambda: pile(alpha=None)), ("null", lambda: pile(idx_m=None)),
           ("null", lambda: pile(out=None)),
           ("n_beads", lambda: L.spk_md_rp_centroid_f32(X, 0, 5, Y, None, 0, 0, None, 0, None)),
           ("n_beads", lambda: L.spk_md_rp_centroid_f32(X, 65, 5, Y, None, 0, 0, None, 0, None)),
           ("null", lambda: L.spk_md_rp_centroid_f32(None, 4, 5, Y, None, 0, 0, None, 0, None)),
           ("alias", lambda: L.spk_md_rp_centroid_f32(X, 4, 5, X, None, 0, 0, None, 0, None)),
           ("null", lambda: L.spk_md_pile_alpha_f32(None, X, X, X, X, 2, 5, 0.9, 0.1, X, None, None)),
           ("c1", lambda: L.spk_md_pile_alpha_f32(X, X, X, X, X, 2, 5, 0.0, 0.1, X, None, None)),
           ("bad sizes", lambda: L.spk_md_pile_alpha_f32(X, X, X, X, X, -1, 5, 0.9, 0.1, X, None, None))]
    for what, call in bad:
        with pytest.raises(SpkHipError, match=what):
            check(call())
    # nothing to do: accepted without touching a pointer
    check(nhc(N=0, p_all=None, out=None))
    check(pile(N=0, p_all=None))
    check(pile(n_local=0, bead0=4, out=None))
