"""CPU: the MD leg against fixtures produced by the REFERENCE's own code -- its PILE-L
thermostat, velocity-Verlet steps, ``Simulator.simulate`` loop and replica folding, lifted and executed by
``oracle/make_golden.py`` (``md_pile``, ``md_verlet``, ``md_simulate``, ``md_fold``).  Pinned here: ``oracle/md_oracle.py`` (the
float64 restatement every GPU test of the MD kernels compares with), the host side of ``schnetpack_amd/md.py`` (coefficients,
mixing matrices, noise scale, folding) and the published known answers of Philox-4x32-10.

The unit constants (kB, fs, hbar) are NOT pinned: the fixtures are generated with the project's values (stored as ``unit_*``).
"""
import numpy as np
import pytest
import torch

from conftest import load_npz, rel_err
from oracle import make_golden as G
from oracle import md_oracle as MDO
from oracle import refshim

U24 = 2.0 ** -24          # half a float32 ulp of a number in [1, 2): the relative rounding error of one float32 operation


def c2_bound(c1, c2):
    """What the reference's float32 ``c2 = sqrt(1 - c1**2)`` may differ by from the exact value.  A relative error e in ``c1**2``
    moves ``1 - c1**2 = c2**2`` by ``c1**2 e``, i.e. c2 by ``c1**2 e / (2 c2)``; the roundings of exp, of the square, and the 4 ulp
    allowed on c1 itself are each at most a few U24.  The subtraction and the square root add relative roundings of c2.  With room
    for four roundings of either kind: |dc2| <= 4 U24 c1^2 / c2 + 4 U24 c2, evaluated with the fixture's c1 and c2 (the reference
    against the float64 port uses at most 0.19 of it; worst relative gap 2.9e-5)."""
    c1, c2 = np.asarray(c1, dtype=np.float64), np.asarray(c2, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(c2 > 0, 4 * U24 * c1 ** 2 / c2 + 4 * U24 * c2, 0.0)


def pile_cases():
    return [(nb, s) for nb in G.PILE_BEADS for s in range(len(G.PILE_SETS))]


@pytest.fixture(scope="module")
def pile():
    return load_npz("md_pile.npz")


# ----------------------------------------------------------------------------- the counter-based generator
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    """The published Random123 test vectors of Philox-4x32-10 (kat_vectors: zero, all ones, digits of pi)."""
    got = MDO.philox4x32_10(*counter, *key)
    assert tuple(int(x) for x in got) == want
    # vectorised over the counter, as pile_noise calls it
    got = MDO.philox4x32_10(*(np.array([c, c], dtype=np.uint64) for c in counter), *key)
    assert all(int(g[0]) == w and int(g[1]) == w for g, w in zip(got, want))


# ----------------------------------------------------------------------------- PILE-L coefficients and application
def test_pile_fixture_covers_the_stated_cases(pile):
    assert tuple(pile["n_beads"]) == (1, 2, 3, 4, 5, 8, 16, 32, 64)
    assert [tuple(r) for r in pile["sets"]] == [(55, 5e-4, 100, 1, 1), (157, 2e-4, 10, 1, 1), (40, 5e-4, 1, 0, 0.5), (314, 5e-4, 1000, 1, 1)]
    from schnetpack_amd import md as MD
    assert (pile["unit_kB"], pile["unit_fs"], pile["unit_hbar"]) == (MD.KB_MD, MD.FS_MD, MD.HBAR_MD)
    m = pile["b8_m"].reshape(-1)
    assert m[0] == 1.008 and m[1] == 200.0 and m[2:].min() >= 1.0 and m[2:].max() <= 16.0 and m.shape == (7,)


@pytest.mark.parametrize("nb,s", pile_cases())
@pytest.mark.parametrize("port", ["oracle", "product"])
def test_pile_coefficients_match_the_reference(pile, nb, s, port):
    """c1 within 4 float32 ulp; c2 within the float32 cancellation of the reference (``c2_bound``); an unthermostatted centroid
    (TRPMD: c1 == 1, c2 == 0 in the reference) must give exactly 0.  Also: omega_normal and the transformer matrix."""
    from schnetpack_amd import md as MD
    omega, dt, tau_fs, centroid, damping = pile["sets"][s]
    t = "b%d_s%d_" % (nb, s)
    fn = MDO.pile_coefficients if port == "oracle" else MD.pile_coefficients
    c1, c2 = fn(nb, float(omega), float(dt), float(tau_fs) * MD.FS_MD, bool(centroid), float(damping))
    assert c1.dtype == torch.float64 and c2.dtype == torch.float64
    r1, r2 = pile[t + "c1"], pile[t + "c2"]
    assert r1.dtype == np.float32 and r2.dtype == np.float32
    d1 = np.abs(c1.numpy() - r1.astype(np.float64))
    assert (d1 <= 4 * np.spacing(r1).astype(np.float64)).all(), (d1, r1)
    d2 = np.abs(c2.numpy() - r2.astype(np.float64))
    bound = c2_bound(r1, r2)
    assert (d2 <= bound).all(), (d2, bound)
    assert (c2.numpy()[r2 == 0] == 0).all()
    if not centroid:
        assert r2[0] == 0 and r1[0] == 1
    on, _ = MDO.ring_polymer_propagator(nb, float(omega), float(dt))
    assert np.array_equal(on.numpy(), pile[t + "omega_normal"])
    Cf = torch.from_numpy(pile["b%d_C" % nb])
    for C in (MDO.normal_mode_matrix(nb), MD.normal_mode_matrix(nb)):
        assert float((C - Cf).abs().max()) < 1e-14


@pytest.mark.parametrize("nb,s", pile_cases())
def test_pile_apply_matches_the_reference_float64_run(pile, nb, s):
    """``md_oracle.pile_apply`` fed the fixture's C, c1, c2 and the noise by (seed, step, which) against the lifted
    ``_apply_thermostat`` on a float64 system: 1e-12.  The float32 run of the reference stays within float32 rounding of it."""
    from schnetpack_amd import md as MD
    t = "b%d_s%d_" % (nb, s)
    p, m, C = (torch.from_numpy(pile["b%d_%s" % (nb, k)]) for k in ("p", "m", "C"))
    c1, c2 = torch.from_numpy(pile[t + "c1"]).double(), torch.from_numpy(pile[t + "c2"]).double()
    xi = MDO.pile_noise(nb, 7, int(pile["seed"]), int(pile["step"]), int(pile["which"]))
    kT = MD.KB_MD * nb * float(pile["temperature"])
    got = MDO.pile_apply(p, m, C, c1, c2, kT, xi)
    ref = torch.from_numpy(pile[t + "f64_p_out"])
    assert rel_err(got, ref) < 1e-12
    assert rel_err(torch.sqrt(m * kT).expand(1, 7, 1), torch.from_numpy(pile[t + "f64_thermostat_factor"])) < 1e-7   # T is a float32 buffer there
    ref32 = torch.from_numpy(pile[t + "f32_p_out"])
    assert ref32.dtype == torch.float32 and rel_err(ref32, ref) < 64 * nb * U24


@pytest.mark.parametrize("nb,s", pile_cases())
def test_thermostat_class_reproduces_the_reference_application(pile, nb, s):
    """``md.PILELocalThermostat`` as the device consumes it -- M = (C^T diag(c1) C, C^T diag(c2)) in float32, ``noise_scale`` and the
    fs conversion of the time constant -- evaluated on the host in float64 the way ``k_md_pile`` does,
    p' = M1 p + sqrt(m) noise_scale M2 xi, against the reference's float64 run.  Tolerance: the device test's
    rtol 2e-5 / atol 2e-5 max|ref|, widened only by the derived c2 term (the reference's own float32 cancellation)."""
    from schnetpack_amd import md as MD
    omega, dt, tau_fs, centroid, damping = (float(x) for x in pile["sets"][s])
    t = "b%d_s%d_" % (nb, s)
    th = MD.PILELocalThermostat(float(pile["temperature"]), tau_fs, bool(centroid), damping).init(MD.RingPolymer(dt, nb, 300.0, omega=omega))
    # the matrices are the float32 rounding of the float64 product with the coefficients
    C = torch.from_numpy(pile["b%d_C" % nb])
    c1, c2 = MD.pile_coefficients(nb, omega, dt, tau_fs * MD.FS_MD, bool(centroid), damping)
    M64 = torch.stack([C.t() @ torch.diag(c1) @ C, C.t() @ torch.diag(c2)])
    assert th.M.dtype == torch.float32 and th.M.shape == (2, nb, nb)
    assert bool(((th.M.double() - M64).abs() <= 2 * U24 * M64.abs() + 1e-13).all())
    p, m = torch.from_numpy(pile["b%d_p" % nb]), torch.from_numpy(pile["b%d_m" % nb])
    xi = MDO.pile_noise(nb, 7, int(pile["seed"]), int(pile["step"]), int(pile["which"]))
    M = th.M.double()
    got = (M[0] @ p.reshape(nb, -1) + M[1] @ (m.sqrt() * th.noise_scale * xi).reshape(nb, -1)).view(p.shape)
    ref = torch.from_numpy(pile[t + "f64_p_out"])
    assert bool(((got - ref).abs() <= pile_tolerance(pile, nb, s, ref, xi)).all()), float((got - ref).abs().max() / ref.abs().max())


def pile_tolerance(pile, nb, s, ref, xi, bead0=0, n_local=None):
    """Elementwise bound of a float32 evaluation against the reference's output: 2e-5 |ref| + 2e-5 max|ref| (the project's bound for
    this kernel) + what the reference's own float32 c2 may be off by, carried through the back-transform:
    sum_k |C[k, b]| thermostat_factor |xi_k| c2_bound_k."""
    t = "b%d_s%d_" % (nb, s)
    C = torch.from_numpy(pile["b%d_C" % nb])
    factor = torch.from_numpy(pile[t + "f64_thermostat_factor"])
    dc2 = torch.from_numpy(c2_bound(pile[t + "c1"], pile[t + "c2"]))
    extra = (C.t().abs() @ (dc2[:, None, None] * factor * xi.abs()).reshape(nb, -1)).view(xi.shape)
    hi = nb if n_local is None else bead0 + n_local
    return 2e-5 * ref.abs() + 2e-5 * float(ref.abs().max()) + extra[bead0:hi]


# ----------------------------------------------------------------------------- integrator steps and the step order
def test_half_step_and_verlet_step_match_the_reference():
    g = load_npz("md_verlet.npz")
    R, p, F, m = (torch.from_numpy(g[k]) for k in ("R", "p", "F", "m"))
    dt = float(g["dt"])
    assert R.shape == (3, 11, 3) and R.dtype == torch.float64
    p1 = MDO.half_step(p, F, dt)
    assert rel_err(p1, torch.from_numpy(g["p_half"])) < 1e-15
    R1 = MDO.verlet_main_step(R, p1, m, dt)
    assert rel_err(R1, torch.from_numpy(g["R_main"])) < 1e-15
    assert rel_err(MDO.half_step(p1, F, dt), torch.from_numpy(g["p_end"])) < 1e-15


EVENTS = ["calculate", "simulation_start recorder", "thermostat", "step_begin recorder", "half_step", "main_step", "calculate",
          "step_middle recorder", "half_step", "step_end recorder", "thermostat", "step_finalize recorder", "simulation_end recorder"]
# measured: the oracle trajectory with float64 coefficients against the same trajectory with the reference's float32-rounded
# coefficients, max over the six steps (see the docstring below); the test allows 4x
SIM_GAP_Q, SIM_GAP_P = 1.1e-9, 2.1e-8


def test_oracle_step_sequence_follows_the_reference_simulator():
    """The NVT ring-polymer step as the GPU tests integrate it through ``md_oracle`` (thermostat, kick, ring-polymer step, forces,
    kick, thermostat; tests/test_gpu_pimd.py) against six steps of the reference's ``Simulator.simulate`` with its RingPolymer and
    PILE-L thermostat (tests/golden/md_simulate.npz).

    * with the reference's own float32 coefficients substituted the oracle reproduces the trajectory to float64 rounding (1e-12);
    * with its own float64 coefficients it differs by the float32 rounding of c1 / c2 only.  Measured gap (max over the steps of
      max|a-b| / max|b|) between those two oracle runs: positions 1.04e-9, momenta 2.07e-8 (SIM_GAP_Q / SIM_GAP_P); 4x that is allowed against the fixture;
    * the thermostat hook is applied before the recorder at step begin and after it at step end (reversed hooks);
    * the two wrong orders stored with the fixture are at least 100x the GPU test's tolerance away, so that test can see them."""
    from schnetpack_amd import md as MD
    g = load_npz("md_simulate.npz")
    assert list(g["events_first_step"]) == EVENTS
    assert (int(g["n_beads"]), int(g["n_steps"]), float(g["dt"]), float(g["omega"]), float(g["tau_fs"]), float(g["temperature"]), int(g["seed"])) == \
        (G.SIM["n_beads"], G.SIM["n_steps"], G.SIM["dt"], G.SIM["omega"], G.SIM["tau_fs"], G.SIM["T"], G.SIM["seed"])
    assert g["c1"].dtype == np.float32 and float(g["c1"][0]) <= 0.98
    setup = G.sim_setup()
    assert torch.equal(setup["q0"], torch.from_numpy(g["q0"])) and torch.equal(setup["p0"], torch.from_numpy(g["p0"]))
    assert G.checksum(setup["rep_p"]) + G.checksum(setup["head_p"]) == float(g["weights_checksum"])
    q_ref, p_ref = torch.from_numpy(g["q"]), torch.from_numpy(g["p"])
    c1f, c2f = torch.from_numpy(g["c1"]).double(), torch.from_numpy(g["c2"]).double()
    q32, p32 = G.sim_oracle_trajectory(setup, c1f, c2f)
    assert max(rel_err(q32[k], q_ref[k]) for k in range(6)) < 1e-12 and max(rel_err(p32[k], p_ref[k]) for k in range(6)) < 1e-12
    c1, c2 = MDO.pile_coefficients(G.SIM["n_beads"], G.SIM["omega"], G.SIM["dt"], G.SIM["tau_fs"] * MD.FS_MD)
    q64, p64 = G.sim_oracle_trajectory(setup, c1, c2)
    gap_q, gap_p = max(rel_err(q64[k], q32[k]) for k in range(6)), max(rel_err(p64[k], p32[k]) for k in range(6))
    print("oracle float64 coefficients vs float32 coefficients: positions %.3e momenta %.3e" % (gap_q, gap_p))
    assert max(rel_err(q64[k], q_ref[k]) for k in range(6)) <= 4 * SIM_GAP_Q
    assert max(rel_err(p64[k], p_ref[k]) for k in range(6)) <= 4 * SIM_GAP_P
    assert 4 * SIM_GAP_Q < 0.1 * float(g["tol_q"]) and 4 * SIM_GAP_P < 0.1 * float(g["tol_p"])      # far below what the GPU test allows
    for order in ("after_first_kick", "before_second_kick"):
        qw, pw = torch.from_numpy(g["wrong_%s_q" % order]), torch.from_numpy(g["wrong_%s_p" % order])
        assert rel_err(qw, q_ref[-1]) >= 100 * float(g["tol_q"]) and rel_err(pw, p_ref[-1]) >= 100 * float(g["tol_p"]), order
    # and the stored wrong end states are what the oracle gives for those orders
    qw, pw = G.sim_oracle_trajectory(setup, c1f, c2f, "before_second_kick")
    assert rel_err(qw[-1], torch.from_numpy(g["wrong_before_second_kick_q"])) < 1e-12


# ----------------------------------------------------------------------------- replica folding
def test_fold_replicas_matches_the_reference_calculator():
    """``md.fold_replicas`` against the lifted ``MDCalculator._get_system_molecules`` (2 replicas x aspirin + ethanol, cells, mixed
    pbc): exact.  The reference hands out pbc as [n_replicas * n_molecules, 3]; the project's batches carry it flat."""
    from schnetpack_amd import md as MD, properties as P
    g = load_npz("md_fold.npz")
    inputs = {P.Z: torch.from_numpy(g["in_Z"]), P.n_atoms: torch.from_numpy(g["in_n_atoms"]), P.idx_m: torch.from_numpy(g["in_idx_m"]),
              P.R: torch.from_numpy(g["in_positions"]), P.cell: torch.from_numpy(g["in_cells"]), P.pbc: torch.from_numpy(g["in_pbc"]).reshape(-1)}
    assert sorted(g["keys"]) == sorted([P.Z, P.n_atoms, P.idx_m, P.R, P.cell, P.pbc])
    assert list(g["in_n_atoms"]) == [21, 9] and int(g["n_replicas"]) == 2
    for pbc in (inputs[P.pbc], inputs[P.pbc].reshape(-1, 3)):
        rep = MD.fold_replicas(dict(inputs, **{P.pbc: pbc}), int(g["n_replicas"]))
        for key, name in ((P.Z, "Z"), (P.n_atoms, "n_atoms"), (P.idx_m, "idx_m"), (P.cell, "cells")):
            want = torch.from_numpy(g[name])
            assert rep[key].dtype == want.dtype and torch.equal(rep[key], want), name
        assert rep[P.pbc].dtype == torch.bool and torch.equal(rep[P.pbc].reshape(-1, 3), torch.from_numpy(g["pbc"]))
        # every replica starts from the given positions (the simulation overwrites them bead by bead)
        assert rep[P.R].shape == g["positions"].shape and torch.equal(rep[P.R], torch.from_numpy(g["positions"]))
    no_cell = {k: v for k, v in inputs.items() if k not in (P.cell, P.pbc)}
    rep = MD.fold_replicas(no_cell, 3)
    assert P.cell not in rep and P.pbc not in rep and int(rep[P.idx_m].max()) == 5 and rep[P.Z].shape[0] == 90


# ----------------------------------------------------------------------------- fixture freshness
def _reference_sources():
    return refshim.available() and not refshim.sourceless()


@pytest.mark.skipif(not _reference_sources(), reason="reference sources not present (the fixtures are regenerated from them)")
@pytest.mark.parametrize("name", G.MD_FIXTURES)
def test_md_fixture_is_what_the_reference_produces_now(name, tmp_path):
    """Regenerate the fixture in memory from the live reference and compare with the committed file: same keys, dtypes, values --
    and the same bytes when written."""
    import os
    from conftest import GOLDEN
    fresh = G.md_arrays(name)
    stored = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    assert sorted(fresh) == sorted(stored.files)
    for k, v in fresh.items():
        v = np.asanyarray(v)
        assert v.dtype == stored[k].dtype and v.shape == stored[k].shape and np.array_equal(v, stored[k]), k
        assert v.dtype.kind in "fiubU", k            # numbers and short tags only
    G.save_npz_reproducible(str(tmp_path / "again.npz"), fresh)
    assert (tmp_path / "again.npz").read_bytes() == open(os.path.join(GOLDEN, name + ".npz"), "rb").read()
