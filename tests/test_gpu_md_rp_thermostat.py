"""GPU: the ring-polymer thermostats of csrc/spk_md_rp_thermo.hip (NHC on the normal modes, PILE-G, TRPMD; ``schnetpack_amd.md``)
against the reference's fixture (tests/golden/md_rp_thermostat.npz) and, for shapes the fixture does not hold, against
tests/md_rp_thermostat_oracle.py.

Tolerances.  NHC-RP: ``allowed_error`` -- 4 x the reference's own float32-versus-float64 gap on the same case (the fixture stores
that gap per compared array), floor 4 float32 ulp of the quantity's magnitude; for oracle-only shapes the gap is that of the oracle evaluated in float32.  PILE-G / TRPMD (noise made
on the device): the project's PILE bound 2e-5 |ref| + 2e-5 max|ref|.  Every test prints what it measured.
"""
import numpy as np
import pytest
import torch

from conftest import load_npz, rel_err
from oracle import md_oracle as MDO
from oracle import spk_oracle as O
from schnetpack_amd import synthetic as S

import md_rp_thermostat_oracle as RO
import md_thermostat_oracle as TO

pytestmark = pytest.mark.gpu
NHC_CASES = ("b1_l3_m2_o3", "b3_l2_m4_o5", "b4_l1_m1_o3")
EMPTIES = [0, 3, 0, 0, 65, 1, 0]        # empty molecules leading, interior and trailing
MANY = [4] * 70                         # more molecules than one 64-thread block


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def g():
    return load_npz("md_rp_thermostat.npz")


def T(x):
    return torch.from_numpy(np.asarray(x))


def layout(sizes):
    n = torch.tensor(sizes, dtype=torch.long)
    return torch.repeat_interleave(torch.arange(len(sizes)), n), n


class St:
    def __init__(self, p, m):
        self.momenta, self.masses = p, m


def pile_ok(dev_p, ref, what):
    ref = ref.double()
    err = (dev_p.double().cpu() - ref).abs()
    bound = 2e-5 * ref.abs() + 2e-5 * float(ref.abs().max())
    worst = float((err / bound).max())
    print("%s: worst error / bound %.3f (max |err| %.3e, max |ref| %.3e)" % (what, worst, float(err.max()), float(ref.abs().max())))
    return worst <= 1.0


# ----------------------------------------------------------------------------- fixture parity
@pytest.mark.parametrize("local", [True, False])
@pytest.mark.parametrize("tag", NHC_CASES)
def test_nhc_rp_matches_the_reference_fixture(dev, g, tag, local):
    from schnetpack_amd import md as MD
    B, L, ms, order = (int(x) for x in g["nhc_params"][list(g["nhc_cases"]).index(tag)])
    name = "nhc_%s_%s" % (tag, "loc" if local else "glo")
    rp = MD.RingPolymer(float(g["dt"]), B, float(g["temperature_bath"]))
    th = MD.NHCRingPolymerThermostat(float(g["temperature_bath"]), float(g["tau_fs"]), local=local, chain_length=L, multi_step=ms,
                                     integration_order=order).init(rp, T(g["idx_m"]), T(g["n_atoms"]))
    st = St(T(g["p_b%d" % B]).float().to(dev), T(g["m_b%d" % B]).float().to(dev))
    for k in range(1, 7):
        th.apply(st)
        if k in (1, 6):
            sd = th.state_dict()
            for key, val in (("p", st.momenta), ("v", sd["velocities"]), ("f", sd["forces"])):
                r64, gap = RO.fixture_nhc(g, tag, local, key, k)
                tol = RO.allowed_error_gap(r64, gap)
                err = float((val.double().cpu() - r64).abs().max())
                print("%s %s after %d: error %.3e allowed %.3e" % (name, key, k, err, tol))
                assert err <= tol, (key, k)
    assert int(th._err.item()) == 0


@pytest.mark.parametrize("B", [1, 3, 4])
def test_pile_global_matches_the_reference_fixture(dev, g, B):
    from schnetpack_amd import md as MD
    rp = MD.RingPolymer(float(g["dt"]), B, float(g["temperature_bath"]))
    th = MD.PILEGlobalThermostat(float(g["temperature_bath"]), float(g["tau_fs"]), seed=int(g["seed"])).init(rp, T(g["idx_m"]), T(g["n_atoms"]))
    st = St(T(g["p_b%d" % B]).float().to(dev), T(g["m_b%d" % B]).float().to(dev))
    for k in range(1, 7):
        th.apply(st, step=k - 1, which=0)
        if k in (1, 6):
            assert pile_ok(st.momenta, RO.fixture_pile(g, "pg_b%d" % B, k), "pile-g B=%d after %d" % (B, k)), k
    assert int(th._err.item()) == 0


def test_pile_global_single_molecule_and_trpmd_match_the_reference_fixture(dev, g):
    from schnetpack_amd import md as MD
    B = int(g["pgs_n_beads"])
    rp = MD.RingPolymer(float(g["dt"]), B, float(g["temperature_bath"]))
    th = MD.PILEGlobalThermostat(float(g["temperature_bath"]), float(g["tau_fs"]), seed=int(g["seed"])).init(rp)     # one molecule of all atoms
    st = St(T(g["p_b%d" % B]).float().to(dev), T(g["m_b%d" % B]).float().to(dev))
    for k in range(1, 7):
        th.apply(st, step=k - 1, which=0)
        if k in (1, 6):
            assert pile_ok(st.momenta, RO.fixture_pile(g, "pgs", k), "pile-g one molecule after %d" % k), k
    for B in (3, 4):
        rp = MD.RingPolymer(float(g["dt"]), B, float(g["temperature_bath"]))
        th = MD.TRPMDThermostat(float(g["temperature_bath"]), float(g["trpmd_damping"]), seed=int(g["seed"])).init(rp)
        st = St(T(g["p_b%d" % B]).float().to(dev), T(g["m_b%d" % B]).float().to(dev))
        for k in range(1, 7):
            th.apply(st, step=k - 1, which=0)
            if k in (1, 6):
                assert pile_ok(st.momenta, RO.fixture_pile(g, "tr_b%d" % B, k), "trpmd B=%d after %d" % (B, k)), k


# ----------------------------------------------------------------------------- shapes where the kernels can go wrong
def thermal(B, N, seed, kT):
    gen = torch.Generator().manual_seed(seed)
    m = (torch.rand(N, generator=gen) * 15 + 1).float()
    p = (torch.randn(B, N, 3, generator=gen) * (m[None, :, None] * kT).sqrt() * 1.4).float()
    return p, m


DT, OMEGA, T0, TAU = 0.01, 3.0, 0.05, 0.2          # unit-free: kb = fs = 1
SHAPES = [(1, [1], 1, True), (2, [85], 3, True), (3, [1367], 6, True), (9, EMPTIES, 3, False), (64, MANY, 3, False), (64, [85], 6, True),
          (9, [1367], 1, False), (2, EMPTIES, 6, False), (3, [1], 3, False)]


@pytest.mark.parametrize("B,sizes,L,local", SHAPES)
def test_nhc_rp_shapes_against_the_oracle(dev, B, sizes, L, local):
    from schnetpack_amd import md as MD
    idx_m, n = layout(sizes)
    N = int(n.sum())
    rp = MD.RingPolymer(DT, B, T0, omega=OMEGA)
    th = MD.NHCRingPolymerThermostat(T0, TAU, local=local, chain_length=L, multi_step=2, integration_order=3, fs=1.0, kb=1.0).init(rp, idx_m, n)
    p, m = thermal(B, N, 5 + B, th.kb_temperature)
    st = St(p.to(dev), m.to(dev))
    C = MDO.normal_mode_matrix(B)
    steps = torch.tensor(th.sub_steps, dtype=torch.float64)
    res = {}
    for dtype in (torch.float64, torch.float32):
        masses = RO.rp_nhc_masses(th.kb_temperature, th.frequencies, RO.rp_nhc_dof(B, idx_m, n, local, torch.float64), L).to(dtype)
        v, f = torch.zeros(B, N, 3, L, dtype=dtype), torch.zeros(B, N, 3, L, dtype=dtype)
        q = p.to(dtype)
        for _ in range(2):
            q = RO.rp_nhc_apply(q, m.to(dtype), idx_m, n, C, th.kb_temperature, masses, v, f, steps.to(dtype), 2, local)
        res[dtype] = (q, v, f)
    th.apply(st)
    th.apply(st)
    sd = th.state_dict()
    for key, val, i in (("p", st.momenta, 0), ("v", sd["velocities"], 1), ("f", sd["forces"], 2)):
        tol = TO.allowed_error(res[torch.float64][i], res[torch.float32][i])
        err = float((val.double().cpu() - res[torch.float64][i]).abs().max())
        print("nhc-rp B=%d N=%d L=%d local=%s %s: error %.3e allowed %.3e" % (B, N, L, local, key, err, tol))
        assert err <= tol, key
    assert int(th._err.item()) == 0
    if not local:          # molecules without atoms keep their (zero) chain
        empty = (n == 0).to(dev)
        assert float(th._cvel[empty].abs().sum()) == 0.0 and bool((th.scaling_factor[empty] == 1).all())


@pytest.mark.parametrize("B,sizes", [(1, [1]), (2, EMPTIES), (3, [85]), (9, MANY), (64, [85]), (3, [1367])])
def test_pile_global_shapes_against_the_oracle(dev, B, sizes):
    from schnetpack_amd import md as MD
    idx_m, n = layout(sizes)
    N = int(n.sum())
    rp = MD.RingPolymer(DT, B, T0, omega=OMEGA)
    th = MD.PILEGlobalThermostat(T0, TAU, seed=11, fs=1.0, kb=1.0).init(rp, idx_m, n)
    p, m = thermal(B, N, 9 + B, th.kb_temperature)
    st = St(p.to(dev), m.to(dev))
    c1, c2 = MD.pile_coefficients(B, OMEGA, DT, TAU)
    q = p.double()
    for step in range(2):
        th.apply(st, step=step, which=1)
        q, alpha = RO.pile_global_apply(q, m.double(), idx_m, n, MDO.normal_mode_matrix(B), c1, c2, th.kb_temperature, MDO.pile_noise(B, N, 11, step, 1))
    print("pile-g alpha: device %s oracle %s" % (th.alpha.cpu()[:4].tolist(), alpha[:4].tolist()))
    assert pile_ok(st.momenta, q, "pile-g B=%d N=%d" % (B, N))
    assert int(th._err.item()) == 0 and bool((th.alpha[(n == 0).to(dev)] == 1).all())


# ----------------------------------------------------------------------------- bead range
@pytest.mark.parametrize("kind", ["nhc_local", "nhc_global", "pile_g"])
def test_a_bead_range_equals_the_rows_of_the_full_call_bit_for_bit(dev, kind):
    from schnetpack_amd import md as MD
    B = 8
    idx_m, n = layout([3, 0, 82])
    rp = MD.RingPolymer(DT, B, T0, omega=OMEGA)

    def make():
        if kind == "pile_g":
            return MD.PILEGlobalThermostat(T0, TAU, seed=5, fs=1.0, kb=1.0).init(rp, idx_m, n)
        return MD.NHCRingPolymerThermostat(T0, TAU, local=kind == "nhc_local", fs=1.0, kb=1.0).init(rp, idx_m, n)
    p, m = thermal(B, 85, 21, B * T0)
    p, m = p.to(dev), m.to(dev)
    full = make()
    first = full.apply_beads(p, m, 0, B, 0, None, 0).clone()
    out = full.apply_beads(first, m, 0, B, 1, None, 1).clone()          # second application: the chains have state
    for lo, nl in ((0, 4), (4, 4), (5, 3)):
        th = make()
        th.apply_beads(p, m, lo, nl, 0, None, 0)
        part = th.apply_beads(first, m, lo, nl, 1, None, 1)
        assert part.shape == (nl, 85, 3) and torch.equal(part, out[lo:lo + nl]), (lo, nl)
        if kind != "pile_g":
            a, b = th.state_dict(), full.state_dict()
            assert torch.equal(a["velocities"], b["velocities"]) and torch.equal(a["forces"], b["forces"]), (lo, nl)


# ----------------------------------------------------------------------------- bit identity
def test_trpmd_is_the_parent_class_bit_for_bit(dev):
    from schnetpack_amd import md as MD
    B = 6
    rp = MD.RingPolymer(DT, B, T0, omega=OMEGA)
    p, m = thermal(B, 85, 3, B * T0)
    a = MD.TRPMDThermostat(T0, 0.7, seed=9, fs=1.0, kb=1.0).init(rp)
    b = MD.PILELocalThermostat(T0, 1.0, thermostat_centroid=False, damping_factor=0.7, seed=9, fs=1.0, kb=1.0).init(rp)
    sa, sb = St(p.to(dev), m.to(dev)), St(p.to(dev), m.to(dev))
    for step in range(3):
        a.apply(sa, step=step, which=1)
        b.apply(sb, step=step, which=1)
    assert torch.equal(sa.momenta, sb.momenta) and not torch.equal(sa.momenta, p.to(dev))


def test_pile_global_modes_are_pile_local_and_a_centroid_at_rest_stays(dev):
    """Input with an exactly zero bead sum (p_{b + B/2} = -p_b, adjacent in the sum): K = 0, alpha = 1, and what is left is PILE-L's
    kernel on the matrices without the centroid -- bit for bit.  An empty molecule in the batch changes nothing."""
    from schnetpack_amd import md as MD
    B = 4
    idx_m, n = layout([0, 40, 0, 45])
    rp = MD.RingPolymer(DT, B, T0, omega=OMEGA)
    p, m = thermal(B, 85, 4, B * T0)
    p[1], p[3] = -p[0], -p[2]
    th = MD.PILEGlobalThermostat(T0, TAU, seed=13, fs=1.0, kb=1.0).init(rp, idx_m, n)
    p, m = p.to(dev), m.to(dev)
    out = th.apply_beads(p, m, 0, B, 2, None, 1)
    ref = MD._pile_hip(p, m, th._M_dev, th.noise_scale, 13, 2, None, 1, 0, B)
    assert bool((th.alpha == 1).all()) and bool(torch.isfinite(out).all())
    assert torch.equal(out, ref)
    cen = out.double().sum(0).abs().max()
    print("centroid at rest after PILE-G: max |sum_b p_b| = %.3e (|p| ~ %.3e)" % (float(cen), float(out.abs().max())))
    assert float(cen) <= 8 * 2.0 ** -23 * float(out.abs().max())
    # zero momenta (the first application of every run)
    z = torch.zeros_like(p)
    out = th.apply_beads(z, m, 0, B, 0, None, 0)
    assert bool(torch.isfinite(out).all()) and bool((th.alpha == 1).all())
    nh = MD.NHCRingPolymerThermostat(T0, TAU, local=False, fs=1.0, kb=1.0).init(rp, idx_m, n)
    out = nh.apply_beads(z, m, 0, B)
    assert bool((out == 0).all()) and all(bool(torch.isfinite(t).all()) for t in nh.state_dict().values())


def test_a_malformed_molecule_index_is_reported_and_never_an_address(dev):
    from schnetpack_amd import md as MD
    B = 2
    rp = MD.RingPolymer(DT, B, T0, omega=OMEGA)
    idx_m, n = layout([5, 5])
    p, m = thermal(B, 10, 2, B * T0)
    for th in (MD.PILEGlobalThermostat(T0, TAU, fs=1.0, kb=1.0).init(rp, idx_m, n), MD.NHCRingPolymerThermostat(T0, TAU, local=False, fs=1.0, kb=1.0).init(rp, idx_m, n)):
        th.prepare(p.to(dev), m.to(dev))
        th._idx_m[7] = 1 << 40
        out = th.apply_beads(p.to(dev), m.to(dev), 0, B)
        assert int(th._err.item()) & 2 and bool(torch.isfinite(out).all())


# ----------------------------------------------------------------------------- chain state in and out, masses, reuse
@pytest.mark.parametrize("local", [True, False])
def test_nhc_rp_state_dict_round_trip_continues_bit_for_bit(dev, local):
    """``state_dict`` -> ``load_state_dict`` into a fresh thermostat, before its buffers exist (kept, loaded at ``prepare``) and after
    (copied into the owned buffers): the next application and the state after it are those of the thermostat that went on."""
    from schnetpack_amd import md as MD
    B, L = 3, 3
    idx_m, n = layout([0, 3, 0, 65, 17])
    rp = MD.RingPolymer(DT, B, T0, omega=OMEGA)

    def make():
        return MD.NHCRingPolymerThermostat(T0, TAU, local=local, chain_length=L, fs=1.0, kb=1.0).init(rp, idx_m, n)
    p, m = thermal(B, 85, 31, B * T0)
    p, m = p.to(dev), m.to(dev)
    a = make()
    q = a.apply_beads(a.apply_beads(p, m, 0, B).clone(), m, 0, B).clone()
    sd = {k: v.cpu() for k, v in a.state_dict().items()}
    assert sd["velocities"].shape == (B, 85, 3, L) and float(sd["velocities"].abs().max()) > 0
    if not local:          # centroid rows: the molecule chains, broadcast over atoms and components
        v0 = sd["velocities"][0]
        assert torch.equal(v0, v0[RO.first_atoms(n)[idx_m]][:, :1].expand(85, 3, L))
    before, after = make(), make()
    before.load_state_dict(sd)                              # no buffers yet
    after.prepare(p, m)
    ptr = after._vel.data_ptr()
    after.load_state_dict(sd)
    assert after._vel.data_ptr() == ptr
    want = a.apply_beads(q, m, 0, B)
    for th in (before, after):
        assert torch.equal(th.apply_beads(q, m, 0, B), want)
        x, y = th.state_dict(), a.state_dict()
        assert all(torch.equal(x[k], y[k]) for k in ("velocities", "forces", "masses"))
    with pytest.raises(ValueError, match="expected shape"):
        after.load_state_dict({"velocities": sd["velocities"][:, :, :, :2], "forces": sd["forces"]})
    with pytest.raises(ValueError, match="masses"):
        after.load_state_dict(dict(sd, masses=2.0 * sd["masses"]))


@pytest.mark.parametrize("kind", ["nhc_global", "pile_g"])
def test_other_masses_or_another_atom_count_are_not_served_from_the_cache(dev, kind):
    """The same thermostat handed other masses of the same shape -- another tensor, or the same one written in place -- uses THEM;
    one initialised without a molecule layout follows another atom count.  Each compared with a fresh thermostat, bit for bit."""
    from schnetpack_amd import md as MD
    B = 2
    rp = MD.RingPolymer(DT, B, T0, omega=OMEGA)

    def make():
        if kind == "pile_g":
            return MD.PILEGlobalThermostat(T0, TAU, seed=3, fs=1.0, kb=1.0).init(rp)
        return MD.NHCRingPolymerThermostat(T0, TAU, local=False, fs=1.0, kb=1.0).init(rp)
    p, m = thermal(B, 85, 41, B * T0)
    p, m = p.to(dev), m.to(dev)
    m0 = m.clone()
    th = make()
    first = th.apply_beads(p, m, 0, B).clone()
    m2 = (3.0 * m).contiguous()
    other = th.apply_beads(p, m2, 0, B).clone()
    m.mul_(3.0)                                              # the first tensor again, now with the values of m2
    again = th.apply_beads(p, m, 0, B).clone()
    if kind == "pile_g":                                     # no state: the same call with the same masses, whichever tensor holds them
        assert torch.equal(other, make().apply_beads(p, m2, 0, B)) and torch.equal(again, other) and not torch.equal(other, first)
    else:                                                    # chains advance: a fresh thermostat fed the same sequence of masses
        ref = make()
        ref.apply_beads(p, m0, 0, B)
        assert torch.equal(other, ref.apply_beads(p, m2, 0, B)) and torch.equal(again, ref.apply_beads(p, m2.clone(), 0, B))
    p9, m9 = thermal(B, 9, 42, B * T0)
    out = th.apply_beads(p9.to(dev), m9.to(dev), 0, B)
    assert th.n_atoms == 9 and torch.equal(out, make().apply_beads(p9.to(dev), m9.to(dev), 0, B))
    given = MD.NHCRingPolymerThermostat(T0, TAU, fs=1.0, kb=1.0).init(rp, *layout([85]))
    with pytest.raises(ValueError, match="idx_m has 85 entries for 9 atoms"):
        given.apply_beads(p9.to(dev), m9.to(dev), 0, B)


# ----------------------------------------------------------------------------- RPMDSimulation
_MODEL = {}


def three_molecules():
    systems = []
    for Z, R in ((S.ASPIRIN_Z, S.ASPIRIN_R), (S.ETHANOL_Z, S.ETHANOL_R), (S.ETHANOL_Z[:6], S.ETHANOL_R[:6])):
        R = np.asarray(R, dtype=np.float64)
        ii, jj = S.neighbor_pairs_open(R, 5.0)
        systems.append({"Z": list(Z), "R": R, "idx_i": ii, "idx_j": jj})
    return S.collate(systems), [21, 9, 6]


def painn(dev):
    from schnetpack_amd import model as M
    if "painn" not in _MODEL:
        model = M.build_model("painn")
        M.load_reference_params(model, O.init_painn_params(), O.init_atomwise_params(128, seed=1))
        _MODEL["painn"] = model.to(dev).eval()
    return _MODEL["painn"]


SIM_DT, SIM_B, SIM_OMEGA = 0.02, 4, 2.0
KINDS = ["pile_l", "pile_g", "trpmd", "nhc_local", "nhc_global"]


def make_thermostat(kind):
    from schnetpack_amd import md as MD
    kw = dict(fs=1.0, kb=1.0)
    return {"pile_l": lambda: MD.PILELocalThermostat(0.05, 0.1, seed=77, **kw), "pile_g": lambda: MD.PILEGlobalThermostat(0.05, 0.1, seed=77, **kw),
            "trpmd": lambda: MD.TRPMDThermostat(0.05, 0.5, seed=77, **kw), "nhc_local": lambda: MD.NHCRingPolymerThermostat(0.05, 0.1, **kw),
            "nhc_global": lambda: MD.NHCRingPolymerThermostat(0.05, 0.1, local=False, **kw)}[kind]()


def rpmd(dev, kind, use_graph):
    from schnetpack_amd import md as MD, model as M
    b, sizes = three_molecules()
    inp = M.batch_to_inputs(b, dev)
    inp["_n_atoms"] = torch.tensor(sizes, device=dev)
    masses = torch.where(b["Z"] == 1, 1.008, torch.where(b["Z"] == 6, 12.011, 15.999))
    sim = MD.RPMDSimulation(painn(dev), inp, masses.to(dev), SIM_DT, SIM_B, cutoff=5.0, temperature=0.05, omega=SIM_OMEGA, cutoff_shell=0.3,
                            use_graph=use_graph, thermostat=make_thermostat(kind))
    gen = torch.Generator().manual_seed(0)
    p0 = 0.3 * torch.randn((SIM_B,) + tuple(b["R"].shape), generator=gen) * masses[None, :, None].sqrt()
    sim.state.momenta.copy_(p0.to(dev))
    return sim, b, masses, p0, sizes


@pytest.mark.parametrize("kind", KINDS)
def test_rpmd_graph_replay_equals_eager_bit_for_bit_and_follows_the_oracle(dev, kind):
    from schnetpack_amd import md as MD
    sim_g, b, masses, p0, sizes = rpmd(dev, kind, True)
    sim_e = rpmd(dev, kind, False)[0]
    assert sim_g.graph is not None and sim_e.graph is None
    idx_m, n = layout(sizes)
    th = sim_e.thermostat
    m64, B, N = masses.double(), SIM_B, len(masses)
    C = MDO.normal_mode_matrix(B)
    _, P = MDO.ring_polymer_propagator(B, SIM_OMEGA, SIM_DT)
    kT = th.kb * B * th.temperature_bath
    if kind.startswith("nhc"):
        local, L = kind == "nhc_local", th.chain_length
        tm = RO.rp_nhc_masses(kT, th.frequencies, RO.rp_nhc_dof(B, idx_m, n, local), L)
        v, f = torch.zeros(B, N, 3, L, dtype=torch.float64), torch.zeros(B, N, 3, L, dtype=torch.float64)
        steps = torch.tensor(th.sub_steps, dtype=torch.float64)
    elif kind == "trpmd":
        c1, c2 = MD.pile_coefficients(B, SIM_OMEGA, SIM_DT, th.time_constant, False, th.damping_factor)
    else:
        c1, c2 = MD.pile_coefficients(B, SIM_OMEGA, SIM_DT, th.time_constant)

    def oracle_thermostat(p, step, which):
        if kind.startswith("nhc"):
            return RO.rp_nhc_apply(p, m64, idx_m, n, C, kT, tm, v, f, steps, th.multi_step, local)
        xi = MDO.pile_noise(B, N, th.seed, step, which)
        if kind == "pile_g":
            return RO.pile_global_apply(p, m64, idx_m, n, C, c1, c2, kT, xi)[0]
        return MDO.pile_apply(p, m64.reshape(1, -1, 1), C, c1, c2, kT, xi)
    q, p = b["R"].double()[None].repeat(B, 1, 1), p0.double()
    F = sim_e.state.forces.cpu().double().view(B, N, 3)
    worst_q = worst_p = 0.0
    for step in range(6):
        sim_e.step(1)
        p = MDO.half_step(oracle_thermostat(p, step, 0), F, SIM_DT)
        q, p = MDO.ring_polymer_main_step(q, p, m64.reshape(1, -1, 1), C, P)
        F = sim_e.state.forces.cpu().double().view(B, N, 3)
        p = oracle_thermostat(MDO.half_step(p, F, SIM_DT), step, 1)
        worst_q, worst_p = max(worst_q, rel_err(sim_e.state.positions.cpu(), q)), max(worst_p, rel_err(sim_e.state.momenta.cpu(), p))
    print("rpmd %s against the oracle on device forces: positions %.3e momenta %.3e" % (kind, worst_q, worst_p))
    assert worst_q < 1e-5 and worst_p < 1e-4
    sim_g.step(6)
    assert int(sim_g._stepc.item()) == 6 and int(sim_e._stepc.item()) == 6 and sim_g.n_captures == 1
    assert torch.equal(sim_g.state.positions, sim_e.state.positions) and torch.equal(sim_g.state.momenta, sim_e.state.momenta)
    for key in ("velocities", "forces"):
        if kind.startswith("nhc"):
            assert torch.equal(sim_g.thermostat.state_dict()[key], sim_e.thermostat.state_dict()[key])
    ref = RO.centroid_temperature(sim_g.state.momenta.cpu().double(), m64, idx_m, n, th.kb)
    ct = sim_g.centroid_temperature()
    print("centroid temperature: device %s oracle %s" % (ct.cpu().tolist(), ref.tolist()))
    assert ct.shape == (3,) and rel_err(ct.cpu(), ref) < 1e-6
    assert rel_err(sim_g.centroid_kinetic_energy().cpu(), 1.5 * n.double() * th.kb * ref) < 1e-6
    assert int(getattr(sim_g.thermostat, "_err", torch.zeros(1)).item()) == 0


def test_pile_local_through_the_dispatch_keeps_its_bits(dev):
    """Existing behaviour: ``RPMDSimulation`` with PILE-L gives the same bits after six steps whether the thermostat is reached
    through ``apply_beads`` or ``_pile_hip`` is called directly with the arguments the simulation used to pass."""
    from schnetpack_amd import md as MD
    a = rpmd(dev, "pile_l", True)[0]
    b = rpmd(dev, "pile_l", False)[0]
    M = b.thermostat.M.to(dev)

    def direct(which):
        th, st = b.thermostat, b.state
        MD._pile_hip(st.momenta, st.masses, M, th.noise_scale, th.seed, 0, b._stepc, which, 0, b.n_beads, b._pt)
        with torch.no_grad():
            st.momenta.copy_(b._pt)
    b._thermostat = direct
    a.step(6)
    b.step(6)
    assert a.n_captures == 1 and int(a._stepc.item()) == 6
    assert torch.equal(a.state.momenta, b.state.momenta) and torch.equal(a.state.positions, b.state.positions)
    assert bool(torch.isfinite(a.state.momenta).all()) and float(a.state.momenta.abs().max()) > 0


def test_rpmd_periodic_run_keeps_chain_state_and_step_counter_across_rebuilds(dev):
    """Periodic 192-atom water box, 4 beads, PaiNN, NHC-RP: hot start, list rebuilds (= graph re-captures) mid-run keep using the
    SAME chain-state and step-counter tensors."""
    from schnetpack_amd import md as MD, model as M
    b = S.water_box(n_side=4, seed=7)
    inp = M.batch_to_inputs(b, dev)
    inp["_n_atoms"] = torch.tensor([b["Z"].shape[0]], device=dev)
    inp["_cell"] = b["cell"].reshape(1, 3, 3).to(dev)
    inp["_pbc"] = torch.tensor([True, True, True], device=dev)
    masses = torch.where(b["Z"] == 1, 1.008, 15.999)
    th = MD.NHCRingPolymerThermostat(0.05, 0.3, local=False, fs=1.0, kb=1.0)
    sim = MD.RPMDSimulation(painn(dev), inp, masses.to(dev), 0.01, 4, cutoff=5.0, temperature=0.05, omega=2.0, cutoff_shell=0.3, thermostat=th)
    gen = torch.Generator().manual_seed(1)
    sim.state.momenta.copy_((0.7 * torch.randn((4,) + tuple(b["R"].shape), generator=gen) * masses[None, :, None].sqrt()).to(dev))
    ptrs = (th._vel.data_ptr(), th._frc.data_ptr(), th._cvel.data_ptr(), sim._stepc.data_ptr())
    t0 = float(sim.centroid_temperature()[0])
    n_steps = 0
    while sim.nl.n_builds < 2 and n_steps < 400:
        sim.step(50)
        n_steps += 50
    assert sim.nl.n_builds >= 2 and sim.n_captures >= 2, (sim.nl.n_builds, sim.n_captures)
    assert int(sim._stepc.item()) == n_steps
    assert ptrs == (th._vel.data_ptr(), th._frc.data_ptr(), th._cvel.data_ptr(), sim._stepc.data_ptr())
    sd = th.state_dict()
    assert all(bool(torch.isfinite(sd[k]).all()) for k in ("velocities", "forces")) and float(sd["velocities"].abs().max()) > 0
    assert bool(torch.isfinite(sim.state.momenta).all()) and bool(torch.isfinite(sim.state.positions).all()) and int(th._err.item()) == 0
    print("rpmd water box: %d steps, %d list builds, %d captures, centroid temperature %.4f -> %.4f" %
          (n_steps, sim.nl.n_builds, sim.n_captures, t0, float(sim.centroid_temperature()[0])))
