"""GPU: the MD step kernels (csrc/spk_md.hip) against fixtures produced by the reference's own code (tests/golden/md_pile.npz,
md_verlet.npz, md_simulate.npz; see tests/test_md_reference.py for what pins the fixtures and the float64 oracle) and, at the
shapes where kernels go wrong, against ``oracle/md_oracle.py`` in float64: up to the advertised bead limits (64 for PILE-L, 96
for the ring polymer, whose > 64-bead launches raise the dynamic-LDS limit), bead sub-ranges, atom counts around a workgroup
edge, systems larger than the grid cap (a second round of the grid-stride loops), the skin flags, and the argument checks."""
import math

import pytest
import torch

from conftest import load_npz, rel_err
from oracle import make_golden as G
from oracle import md_oracle as MDO
from test_md_reference import pile_tolerance

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    return torch.device("cuda", 0)


def grid_cap(dev):
    """Work items one launch of the MD kernels covers without going round its grid-stride loop:
    (multi_processor_count * 8) blocks of 256 threads."""
    return torch.cuda.get_device_properties(dev).multi_processor_count * 8 * 256


def flag_words(flag):
    """(moved bit, largest one-step displacement) of a skin flag."""
    return int(flag[0].item()), math.sqrt(flag[1:].view(torch.float32).item())


# ----------------------------------------------------------------------------- PILE-L
@pytest.mark.parametrize("s", range(len(G.PILE_SETS)))
@pytest.mark.parametrize("nb", G.PILE_BEADS)
def test_pile_kernel_matches_the_reference_output_on_the_same_noise(dev, nb, s):
    """spk_md_pile_f32 (matrices and noise scale from ``PILELocalThermostat``) against the momenta the reference's own
    ``_apply_thermostat`` produced from the same normal-mode noise -- its float64-system run and its float32 run.  Tolerance:
    rtol 2e-5, atol 2e-5 max|ref| (tests/test_gpu_md.py), widened only by the reference's own float32 error in c2."""
    from schnetpack_amd import md as MD
    pile = load_npz("md_pile.npz")
    omega, dt, tau_fs, centroid, damping = (float(x) for x in pile["sets"][s])
    t = "b%d_s%d_" % (nb, s)
    th = MD.PILELocalThermostat(float(pile["temperature"]), tau_fs, bool(centroid), damping, seed=int(pile["seed"]))
    th.init(MD.RingPolymer(dt, nb, 300.0, omega=omega))
    p, m = torch.from_numpy(pile["b%d_p" % nb]), torch.from_numpy(pile["b%d_m" % nb])
    got = MD._pile_hip(p.float().to(dev), m.float().to(dev), th.M.to(dev), th.noise_scale, th.seed, int(pile["step"]), None,
                       int(pile["which"]), 0, nb).cpu().double()
    xi = MDO.pile_noise(nb, 7, int(pile["seed"]), int(pile["step"]), int(pile["which"]))
    for run in ("f64", "f32"):
        ref = torch.from_numpy(pile[t + run + "_p_out"]).double()
        err = (got - ref).abs()
        print("pile nb=%d set=%d vs %s: max err / max|ref| = %.3e" % (nb, s, run, float(err.max() / ref.abs().max())))
        assert bool((err <= pile_tolerance(pile, nb, s, ref, xi)).all()), (run, float(err.max() / ref.abs().max()))
    # through the class, with the step on the device
    st = MD.MDState(None, p.float().to(dev), m.float().to(dev), forces=p.float().to(dev))
    stepc = torch.tensor([int(pile["step"])], dtype=torch.int64, device=dev)
    assert torch.equal(th.apply(st, 0, int(pile["which"]), step_dev=stepc).cpu().double(), got)


PILE_RANGES = [(1, 0, 1), (2, 0, 2), (3, 1, 2), (8, 0, 8), (9, 0, 9), (17, 0, 17), (32, 8, 16), (64, 0, 64), (64, 63, 1)]


def _pile_case(dev, nb, bead0, n_local, n_atoms, gen_seed=5):
    from schnetpack_amd import md as MD
    g = torch.Generator().manual_seed(gen_seed + nb + n_atoms % 1000)
    omega, dt, tau, T = 55.0, 5e-4, 0.1, 300.0
    p = torch.randn(nb, n_atoms, 3, generator=g)
    masses = torch.rand(1, n_atoms, 1, generator=g) * 15 + 1
    M = MD.pile_matrices(nb, omega, dt, tau)
    seed, step, which = 0x1234567ABCDEF, 41, 1
    out = torch.full((max(n_local, 1), n_atoms, 3), float("nan"), device=dev)
    got = MD._pile_hip(p.to(dev), masses.to(dev), M.to(dev), math.sqrt(MD.KB_MD * nb * T), seed, step, None, which, bead0, n_local, out).cpu()
    C = MDO.normal_mode_matrix(nb)
    c1, c2 = MDO.pile_coefficients(nb, omega, dt, tau)
    xi = MDO.pile_noise(nb, n_atoms, seed, step, which)
    ref = MDO.pile_apply(p.double(), masses.double(), C, c1, c2, MD.KB_MD * nb * T, xi)[bead0:bead0 + n_local]
    return got, ref


@pytest.mark.parametrize("n_atoms", [1, 21, 85, 86])
@pytest.mark.parametrize("nb,bead0,n_local", PILE_RANGES)
def test_pile_kernel_shapes(dev, nb, bead0, n_local, n_atoms):
    """Bead counts up to the limit of 64, sub-ranges that start inside a PILE_CHUNK pass and end on the last bead, odd counts (the
    unpaired last mode of a Philox block), 85 / 86 atoms = 255 / 258 work items around the workgroup edge: against md_oracle in
    float64 at the project's rtol 2e-5, atol 2e-5 max|ref|."""
    got, ref = _pile_case(dev, nb, bead0, n_local, n_atoms)
    assert got.shape == ref.shape
    print("pile shape nb=%d [%d,+%d) atoms=%d: %.3e" % (nb, bead0, n_local, n_atoms, rel_err(got, ref)))
    assert torch.allclose(got.double(), ref, rtol=2e-5, atol=2e-5 * float(ref.abs().max()))


@pytest.mark.parametrize("nb,bead0,n_local", [(2, 0, 2), (8, 0, 8), (8, 5, 3)])
def test_pile_kernel_beyond_one_grid(dev, nb, bead0, n_local):
    """3 n_atoms work items exceed the grid cap: every thread goes round the grid-stride loop a second time for some of them."""
    cap = grid_cap(dev)
    n_atoms = cap // 3 + 1000
    assert 3 * n_atoms > cap
    got, ref = _pile_case(dev, nb, bead0, n_local, n_atoms)
    assert torch.allclose(got.double(), ref, rtol=2e-5, atol=2e-5 * float(ref.abs().max()))
    tail = slice(cap // 3 - 2, None)          # the work items of the second round
    assert torch.allclose(got[:, tail].double(), ref[:, tail], rtol=2e-5, atol=2e-5 * float(ref.abs().max()))


def test_pile_kernel_with_no_local_beads_writes_nothing(dev):
    from schnetpack_amd import md as MD
    p = torch.randn(4, 50, 3, device=dev)
    out = torch.full((1, 50, 3), float("nan"), device=dev)
    MD._pile_hip(p, torch.ones(50, device=dev), MD.pile_matrices(4, 55.0, 5e-4, 0.1).to(dev), 1.0, 1, 0, None, 0, 2, 0, out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ----------------------------------------------------------------------------- ring-polymer main step
def _rp_case(nb, n_atoms, seed=0):
    from schnetpack_amd import md as MD
    gen = torch.Generator().manual_seed(1000 * seed + nb)
    omega, dt = 40.0 + 3.0 * nb, 5e-4
    Q, Pm = torch.randn(nb, n_atoms, 3, generator=gen), torch.randn(nb, n_atoms, 3, generator=gen)
    Mass = torch.rand(1, n_atoms, 1, generator=gen) * 15 + 1
    A = MD.ring_polymer_matrices(nb, omega, dt)
    C = MDO.normal_mode_matrix(nb)
    _, prop = MDO.ring_polymer_propagator(nb, omega, dt)
    q2, p2 = MDO.ring_polymer_main_step(Q.double(), Pm.double(), Mass.double(), C, prop)
    return Q, Pm, Mass, A, q2, p2


def test_ring_polymer_bead_counts_up_to_the_limit(dev):
    """1 .. 96 beads, 257 atoms (one thread into a second workgroup), against ``md_oracle.ring_polymer_main_step`` at 1e-5; full
    range and sub-ranges incl. ``bead0 + n_local == n_beads``.  64 beads is the last launch inside the default dynamic-LDS
    limit; 65 and 96 raise it (hipFuncSetAttribute, once per device); 8 beads afterwards checks the small launch still works
    once the attribute is set."""
    from schnetpack_amd.md import _ring_polymer_hip
    for nb in (1, 2, 3, 16, 33, 64, 65, 96, 8):
        Q, Pm, Mass, A, q2, p2 = _rp_case(nb, 257)
        Qd, Pd, Md, Ad = Q.to(dev), Pm.to(dev), Mass.to(dev), A.to(dev)
        for lo, hi in sorted({(0, nb), (nb // 2, nb), (nb // 3, max(nb // 3 + 1, nb - 1)), (nb - 1, nb)}):
            qo, po = _ring_polymer_hip(Qd, Pd, Md, Ad, lo, hi - lo)
            eq, ep = rel_err(qo.cpu(), q2[lo:hi]), rel_err(po.cpu(), p2[lo:hi])
            print("ring polymer nb=%d [%d,%d): q %.3e p %.3e" % (nb, lo, hi, eq, ep))
            assert qo.shape == (hi - lo, 257, 3) and eq < TOL and ep < TOL, (nb, lo, hi, eq, ep)


def test_ring_polymer_beyond_one_grid(dev):
    """More atoms than the grid cap (one thread per atom): the second round of the grid-stride loop, 2 beads."""
    from schnetpack_amd.md import _ring_polymer_hip
    cap = grid_cap(dev)
    n_atoms = cap + 777
    assert n_atoms > cap
    Q, Pm, Mass, A, q2, p2 = _rp_case(2, n_atoms)
    for lo, hi in ((0, 2), (1, 2)):
        qo, po = _ring_polymer_hip(Q.to(dev), Pm.to(dev), Mass.to(dev), A.to(dev), lo, hi - lo)
        assert rel_err(qo.cpu(), q2[lo:hi]) < TOL and rel_err(po.cpu(), p2[lo:hi]) < TOL
        assert rel_err(qo.cpu()[:, cap - 2:], q2[lo:hi, cap - 2:]) < TOL and rel_err(po.cpu()[:, cap - 2:], p2[lo:hi, cap - 2:]) < TOL


# ----------------------------------------------------------------------------- skin flags
def _disp_tol(n_terms, scale):
    """Absolute error of a float32 position that is a sum of ``n_terms`` fused multiply-adds of magnitude ``scale`` (one rounding of
    2^-24 relative each), plus the roundings of the subtraction and of the three squares: (n_terms + 4) 2^-23 scale."""
    return (n_terms + 4) * 2.0 ** -23 * scale


@pytest.mark.parametrize("where", ["local", "non_local"])
def test_ring_polymer_skin_flag_of_a_bead_sub_range(dev, where):
    """``flag[0]``: some LOCAL bead moved further than the threshold from ``R_ref`` -- which holds the local beads only and is indexed
    by the local bead, while the one-step displacement ``flag[1]`` compares with the global bead of ``q_all``.  6 beads, the rank
    owns beads 2..4.  "local": the largest displacement (and the largest single step) sits in a local bead; "non_local": a larger
    one sits in a bead of another rank and must be ignored.  Thresholds at 0.99x / 1.01x of the float64 displacement; the flag
    accumulates over calls until it is reset."""
    from schnetpack_amd.md import _ring_polymer_hip
    nb, bead0, n_local, n = 6, 2, 3, 300
    Q, Pm, Mass, A, q2, p2 = _rp_case(nb, n, seed=3)
    big_bead, big_atom = (3, 123) if where == "local" else (0, 123)
    Pm[big_bead, big_atom] = torch.tensor([900.0, -700.0, 800.0]) * float(Mass[0, big_atom, 0]) / 16.0
    C = MDO.normal_mode_matrix(nb)
    _, prop = MDO.ring_polymer_propagator(nb, 40.0 + 3.0 * nb, 5e-4)
    q2, p2 = MDO.ring_polymer_main_step(Q.double(), Pm.double(), Mass.double(), C, prop)
    step = (q2 - Q.double()).norm(dim=-1)            # [B, n] one-step displacement
    loc = slice(bead0, bead0 + n_local)
    if where == "local":
        assert int(step.max(dim=1).values.argmax()) == big_bead and bead0 <= big_bead < bead0 + n_local
    else:
        assert float(step[big_bead].max()) > 1.5 * float(step[loc].max())
    # reference positions of ALL beads: new position minus a known offset, the largest offset in ``big_bead``
    gen = torch.Generator().manual_seed(9)
    delta = torch.randn(nb, n, 3, generator=gen, dtype=torch.float64)
    delta = 0.2 * delta / delta.norm(dim=-1, keepdim=True) * torch.rand(nb, n, 1, generator=gen, dtype=torch.float64)
    delta[big_bead, 77] = torch.tensor([0.3, -0.3, 0.2])
    R_full = (q2 - delta).float()
    disp = (q2 - R_full.double()).norm(dim=-1)
    assert int(disp.max(dim=1).values.argmax()) == big_bead
    d_loc, s_loc = float(disp[loc].max()), float(step[loc].max())
    if where == "non_local":
        assert float(disp.max()) > 1.3 * d_loc
    R_ref = R_full[loc].contiguous().to(dev)
    Qd, Pd, Md, Ad = Q.to(dev), Pm.to(dev), Mass.to(dev), A.to(dev)
    tol_s = _disp_tol(2 * nb, float(q2.abs().max()))
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    qo, po = _ring_polymer_hip(Qd, Pd, Md, Ad, bead0, n_local, None, None, R_ref, 1.01 * d_loc, flag)
    assert rel_err(qo.cpu(), q2[loc]) < TOL and rel_err(po.cpu(), p2[loc]) < TOL
    moved, s = flag_words(flag)
    print("ring polymer flag (%s): step %.6e vs %.6e (tol %.1e), displacement %.4f" % (where, s, s_loc, tol_s, d_loc))
    assert moved == 0 and abs(s - s_loc) <= tol_s
    # a second call with smaller steps and a threshold just below the displacement: the bit comes up, the running maximum stays
    q2b, _ = MDO.ring_polymer_main_step(Q.double(), 0.5 * Pm.double(), Mass.double(), C, prop)
    d_b = float((q2b[loc] - R_full[loc].double()).norm(dim=-1).max())
    s_b = float((q2b[loc] - Q[loc].double()).norm(dim=-1).max())
    alone = torch.zeros(2, dtype=torch.int32, device=dev)          # the second call on a flag of its own
    _ring_polymer_hip(Qd, (0.5 * Pm).to(dev), Md, Ad, bead0, n_local, None, None, R_ref, 1.01 * d_b, alone)
    moved, s = flag_words(alone)
    assert moved == 0 and abs(s - s_b) <= tol_s
    running = max(int(flag[1].item()), int(alone[1].item()))       # non-negative floats order like their bit patterns
    _ring_polymer_hip(Qd, (0.5 * Pm).to(dev), Md, Ad, bead0, n_local, None, None, R_ref, 0.99 * d_b, flag)
    assert flag_words(flag)[0] == 1 and int(flag[1].item()) == running
    # the bit is sticky: a call that sees no displacement above its threshold leaves it
    _ring_polymer_hip(Qd, (0.5 * Pm).to(dev), Md, Ad, bead0, n_local, None, None, R_ref, 1.01 * d_b, flag)
    assert flag_words(flag)[0] == 1 and int(flag[1].item()) == running
    flag.zero_()
    _ring_polymer_hip(Qd, Pd, Md, Ad, bead0, n_local, None, None, R_ref, 0.99 * d_loc, flag)
    assert flag_words(flag)[0] == 1


def test_skin_threshold_is_strict(dev):
    """The criterion is ``|R - R_ref|^2 > max_displacement^2``: an atom exactly ON the threshold has not moved.  Both kernels, with
    positions that do not change (zero momenta; one bead, whose propagator leaves q untouched then) and an offset of exactly
    0.5 in exactly representable numbers."""
    from schnetpack_amd import md as MD
    n = 700
    R = (torch.arange(3 * n, dtype=torch.float32).reshape(1, n, 3) % 64) / 8.0
    R_ref = R.clone()
    R_ref[0, 333, 1] -= 0.5
    R_ref[0, 5, 0] += 0.25
    m = torch.full((1, n, 1), 2.0)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    st = MD.MDState(R.to(dev).clone(), torch.zeros(1, n, 3, device=dev), m.to(dev))
    MD.VelocityVerlet(0.125).first_half_and_main_step(st, False, R_ref.to(dev).reshape(-1, 3).contiguous(), 0.5, flag)
    assert torch.equal(st.positions.cpu(), R) and flag.tolist() == [0, 0]
    MD.VelocityVerlet(0.125).first_half_and_main_step(st, False, R_ref.to(dev).reshape(-1, 3).contiguous(), 0.4999999, flag)
    assert flag.tolist() == [1, 0]
    flag.zero_()
    A = MD.ring_polymer_matrices(1, 30.0, 0.125).to(dev)
    qo, po = MD._ring_polymer_hip(R.to(dev), torch.zeros(1, n, 3, device=dev), m.to(dev), A, 0, 1, None, None, R_ref.to(dev), 0.5, flag)
    assert torch.equal(qo.cpu(), R) and flag.tolist() == [0, 0]
    MD._ring_polymer_hip(R.to(dev), torch.zeros(1, n, 3, device=dev), m.to(dev), A, 0, 1, None, None, R_ref.to(dev), 0.4999999, flag)
    assert flag.tolist() == [1, 0]


@pytest.mark.parametrize("kick", [True, False])
@pytest.mark.parametrize("size", ["small", "beyond_one_grid"])
def test_kick_drift_skin_flag(dev, kick, size):
    """spk_md_kick_drift_f32: positions / momenta against md_oracle, ``flag[0]`` at 0.99x / 1.01x of the float64 displacement,
    ``flag[1]`` against the float64 largest step, accumulation over two calls; with and without the kick (``F = None``), and for
    a system above the grid cap whose extreme atom is the LAST one (reached in the second round of the grid-stride loop)."""
    from schnetpack_amd import md as MD
    n = 1000 if size == "small" else grid_cap(dev) + 513
    if size != "small":
        assert n > grid_cap(dev)
    g = torch.Generator().manual_seed(17)
    R, p, F = (torch.randn(1, n, 3, generator=g) for _ in range(3))
    m = torch.rand(1, n, 1, generator=g) * 15 + 1
    dt = 0.05
    last = n - 1
    p[0, last] = torch.tensor([300.0, 200.0, -250.0]) * float(m[0, last, 0]) / 16.0     # the largest step by far
    p1 = MDO.half_step(p.double(), F.double(), dt) if kick else p.double()
    R1 = MDO.verlet_main_step(R.double(), p1, m.double(), dt)
    step = (R1 - R.double()).norm(dim=-1)
    assert int(step.argmax()) == last
    delta = torch.randn(1, n, 3, generator=g, dtype=torch.float64)
    delta = 0.2 * delta / delta.norm(dim=-1, keepdim=True) * torch.rand(1, n, 1, generator=g, dtype=torch.float64)
    delta[0, last] = torch.tensor([0.3, 0.3, -0.2])
    R_ref = (R1 - delta).float()
    disp = (R1 - R_ref.double()).norm(dim=-1)
    assert int(disp.argmax()) == last
    d, s_max = float(disp.max()), float(step.max())
    ref_dev = R_ref.to(dev).reshape(-1, 3).contiguous()
    vv = MD.VelocityVerlet(dt)
    tol_s = _disp_tol(2, float(R1.abs().max()))
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    st = MD.MDState(R.to(dev).clone(), p.to(dev).clone(), m.to(dev), F.to(dev))
    vv.first_half_and_main_step(st, kick, ref_dev, 1.01 * d, flag)
    assert rel_err(st.positions.cpu(), R1) < 1e-6 and rel_err(st.momenta.cpu(), p1) < 1e-6
    moved, s = flag_words(flag)
    print("kick-drift flag (kick=%s, %s): step %.6e vs %.6e (tol %.1e)" % (kick, size, s, s_max, tol_s))
    assert moved == 0 and abs(s - s_max) <= tol_s
    bits = int(flag[1].item())
    # second call from a calmer state, threshold below ITS displacement: the bit comes up, the running maximum stays
    p_b = p.clone()
    p_b[0, last] *= 0.5
    p1b = MDO.half_step(p_b.double(), F.double(), dt) if kick else p_b.double()
    R1b = MDO.verlet_main_step(R.double(), p1b, m.double(), dt)
    d_b = float((R1b - R_ref.double()).norm(dim=-1).max())
    st = MD.MDState(R.to(dev).clone(), p_b.to(dev).clone(), m.to(dev), F.to(dev))
    vv.first_half_and_main_step(st, kick, ref_dev, 0.99 * d_b, flag)
    assert flag_words(flag)[0] == 1 and int(flag[1].item()) == bits
    flag.zero_()
    st = MD.MDState(R.to(dev).clone(), p.to(dev).clone(), m.to(dev), F.to(dev))
    vv.first_half_and_main_step(st, kick, ref_dev, 0.99 * d, flag)
    assert flag_words(flag)[0] == 1


# ----------------------------------------------------------------------------- reference fixtures of the steps and of the loop
def test_velocity_verlet_matches_the_reference_steps(dev):
    """``VelocityVerlet`` (half step, main step, half step; and the fused first two) against the reference's own ``half_step`` /
    ``_main_step`` on the [3, 11, 3] state of tests/golden/md_verlet.npz."""
    from schnetpack_amd import md as MD
    g = load_npz("md_verlet.npz")
    R, p, F, m = (torch.from_numpy(g[k]).float().to(dev) for k in ("R", "p", "F", "m"))
    vv = MD.VelocityVerlet(float(g["dt"]))
    st = MD.MDState(R.clone(), p.clone(), m, F)
    vv.half_step(st)
    assert rel_err(st.momenta.cpu(), torch.from_numpy(g["p_half"])) < 1e-6
    vv.main_step(st)
    assert rel_err(st.positions.cpu(), torch.from_numpy(g["R_main"])) < 1e-6 and rel_err(st.momenta.cpu(), torch.from_numpy(g["p_half"])) < 1e-6
    vv.half_step(st)
    assert rel_err(st.momenta.cpu(), torch.from_numpy(g["p_end"])) < 1e-6
    st = MD.MDState(R.clone(), p.clone(), m, F)
    vv.first_half_and_main_step(st)
    assert rel_err(st.positions.cpu(), torch.from_numpy(g["R_main"])) < 1e-6 and rel_err(st.momenta.cpu(), torch.from_numpy(g["p_half"])) < 1e-6


def test_rpmd_nvt_steps_follow_the_reference_simulator(dev):
    """``RPMDSimulation`` with ``PILELocalThermostat`` for 6 graph-replayed steps against the trajectory of the reference's
    ``Simulator.simulate`` (its RingPolymer, its PILE-L thermostat as a hook, float64 oracle forces, the same counter-based noise):
    tests/golden/md_simulate.npz.  Positions at 1e-5, momenta at 1e-4 after EVERY step.  This pins the order of
    ``RPMDSimulation._step_body``: the fixture's two wrong orders are >= 100x these bounds away (tests/test_md_reference.py)."""
    from schnetpack_amd import md as MD, model as M
    g = load_npz("md_simulate.npz")
    setup = G.sim_setup()
    b, masses = setup["b"], setup["masses"]
    model = M.build_model("schnet")
    M.load_reference_params(model, setup["rep_p"], setup["head_p"])
    model = model.to(dev).eval()
    inp = M.batch_to_inputs(b, dev)
    inp["_n_atoms"] = torch.full((2,), 21, device=dev)
    B, n_steps = int(g["n_beads"]), int(g["n_steps"])
    th = MD.PILELocalThermostat(float(g["temperature"]), float(g["tau_fs"]), seed=int(g["seed"]))
    sim = MD.RPMDSimulation(model, inp, masses.to(dev), float(g["dt"]), B, cutoff=5.0, omega=float(g["omega"]), cutoff_shell=0.4, thermostat=th)
    sim.state.positions.copy_(torch.from_numpy(g["q0"]).to(dev))
    sim.state.momenta.copy_(torch.from_numpy(g["p0"]).to(dev))
    sim._rebuild(True)
    sim._force_eval()
    q_ref, p_ref = torch.from_numpy(g["q"]), torch.from_numpy(g["p"])
    assert float(g["tol_q"]) == 1e-5 and float(g["tol_p"]) == 1e-4
    for k in range(n_steps):
        sim.step(1)
        eq, ep = rel_err(sim.state.positions.cpu(), q_ref[k]), rel_err(sim.state.momenta.cpu(), p_ref[k])
        print("rpmd nvt step %d: positions %.3e momenta %.3e" % (k + 1, eq, ep))
        assert eq < 1e-5 and ep < 1e-4, (k, eq, ep)
    assert int(sim._stepc.item()) == n_steps and sim.graph is not None


# ----------------------------------------------------------------------------- argument checks
def test_argument_checks_raise_and_launch_nothing(dev):
    """97 beads (ring polymer), 65 beads (PILE-L), a bead range past the end, outputs that alias the inputs: ``SpkHipError`` each,
    and the NaN-filled outputs stay untouched."""
    from schnetpack_amd import md as MD
    from schnetpack_amd._lib import SpkHipError
    n = 40
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    m = torch.ones(n, device=dev)

    def rp(nb, bead0, n_local, q_out=None, p_out=None, q=None, p=None):
        q = torch.randn(nb, n, 3, device=dev) if q is None else q
        p = torch.randn(nb, n, 3, device=dev) if p is None else p
        return MD._ring_polymer_hip(q, p, m, torch.zeros(4, nb, nb, device=dev), bead0, n_local, q_out, p_out)

    qo, po = nan(2, n, 3), nan(2, n, 3)
    with pytest.raises(SpkHipError, match="n_beads <= 96"):
        rp(97, 0, 2, qo, po)
    with pytest.raises(SpkHipError, match="bead range"):
        rp(8, 7, 2, qo, po)
    with pytest.raises(SpkHipError, match="bead range"):
        rp(8, -1, 2, qo, po)
    q = torch.randn(2, n, 3, device=dev)
    q_before = q.clone()
    with pytest.raises(SpkHipError, match="alias"):
        rp(2, 0, 2, q, po, q=q)
    with pytest.raises(SpkHipError, match="alias"):
        rp(2, 0, 2, qo, q, p=q)

    def pile(nb, bead0, n_local, p_out, p=None):
        p = torch.randn(nb, n, 3, device=dev) if p is None else p
        return MD._pile_hip(p, m, torch.zeros(2, nb, nb, device=dev), 1.0, 1, 0, None, 0, bead0, n_local, p_out)

    with pytest.raises(SpkHipError, match="n_beads <= 64"):
        pile(65, 0, 2, po)
    with pytest.raises(SpkHipError, match="bead range"):
        pile(8, 7, 2, po)
    with pytest.raises(SpkHipError, match="alias"):
        pile(2, 0, 2, q, p=q)
    torch.cuda.synchronize()
    assert bool(torch.isnan(qo).all()) and bool(torch.isnan(po).all()) and torch.equal(q, q_before)
