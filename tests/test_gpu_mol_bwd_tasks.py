"""Derivative tasks of the molecule-resident SchNet backward (csrc/spk_schnet_mol.hip, phase E): one task per pair tile (the filter
hidden layer once, a loop over the two channel-tile pairs behind it) or two tasks per tile, chosen by
``spk_schnet_mol_set_bwd_task_split`` (0 = automatic, 1, 2).

Shapes: groups of exactly 32 atoms (a cluster of ``mol_capacity_cases.capped`` filled up with single atoms, so the plan cannot merge
across them) with 1, 32, 33, 128, 129, 160, 256, 257 and 384 pairs -- 1, 1, 2, 4, 5, 5, 8, 9 and 12 tiles: a full and a one-pair last
tile, fewer tasks than waves, exactly eight tasks, a second round, the capacity -- and a group of 32 single atoms, which has no pair.
The units repeat in a fixed cycle until there are more groups than compute units, so some workgroups take a second, unlike group.

Metric and bounds as in tests/test_gpu_mol_capacity.py: per molecule against the float64 oracle 1e-5, between two device paths 5e-6 on
forces; two task splits on one batch 1e-6 of max|F| (paths whose summation order is not fixed).  With one task per tile
every per-pair sum is built by one wave in one order: bit-reproducible forces.  Every figure is printed before it is asserted."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mol_capacity_cases as C
from oracle import spk_oracle as O
from schnetpack_amd import synthetic as S

pytestmark = pytest.mark.gpu
TOL = 1e-5                      # against the float64 oracle
X_FORCES = 5e-6                 # between two device paths
X_SPLIT = 1e-6                  # between the two task splits, of max |F|
PAIRS = (1, 32, 33, 128, 129, 160, 256, 257, 384)
ATOMS = {1: 2, 32: 9, 33: 9, 128: 17, 129: 17, 160: 19, 256: 24, 257: 24, 384: 32}     # n (n - 1) / 2 >= P
CYCLE = (0,) + PAIRS            # 0: the group of single atoms; 256 groups later a workgroup meets the unit six places on
# cluster seeds: 600 + P, except for the dimer.  A single pair averages nothing: with seed 601 it sits 2.48 A apart, where the
# 8-Gaussian model has a force of 1e-3 (near a zero of its pair force), and the float32 ORACLE is 2e-5 away from the float64 one.
# Seed 622 is the one of 600 ... 639 on which the float32 oracle is closest to the float64 oracle over the three bases, forces and
# dL/dR (7.8e-7; forces of 0.04 ... 0.2).  tests/test_mol_bwd_task_cases.py (CPU) pins 3e-6 for every input used here.
SEEDS = {P: 600 + P for P in PAIRS}
SEEDS[1] = 622


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------
# inputs and references
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _unit(P):
    """Systems of one group of exactly 32 atoms with P pairs."""
    if P == 0:
        return tuple(C.atom(900 + k) for k in range(C.MAX_ATOMS))
    n = ATOMS[P]
    return (C.capped(n, P, SEEDS[P]),) + tuple(C.atom(700 + k) for k in range(C.MAX_ATOMS - n))


def _collate(units):
    systems = [s for P in units for s in _unit(P)]
    b = S.collate(systems)
    plan = C.plan(b)
    want = [0 if P == 0 else P for P in units]
    assert np.diff(plan["grp_atom0"]).tolist() == [C.MAX_ATOMS] * len(units), "one group per unit"
    assert np.diff(plan["grp_pair0"]).tolist() == want, "pairs per group"
    return b


@functools.lru_cache(maxsize=None)
def _distinct_batch():
    return _collate(CYCLE)


@functools.lru_cache(maxsize=None)
def _params(n_rbf):
    return O.init_schnet_params(128, 3, n_rbf, C.CUTOFF), O.init_atomwise_params(128, seed=1)


@functools.lru_cache(maxsize=None)
def _model(n_rbf):
    from schnetpack_amd import model as M
    rep, head = _params(n_rbf)
    m = M.build_model("schnet", 128, 3, n_rbf, C.CUTOFF)
    M.load_reference_params(m, rep, head)
    return m.to(torch.device("cuda:0")).eval()


@functools.lru_cache(maxsize=None)
def _reference(n_rbf):
    """float64 oracle of the ten distinct units (computed once; never modified)."""
    rep, head = _params(n_rbf)
    return O.energy_and_forces("schnet", rep, head, _distinct_batch(), 3, dtype=torch.float64)


def _set_tasks(v):
    from schnetpack_amd import _lib
    _lib.lib().spk_schnet_mol_set_bwd_task_split(ctypes.c_int(v))


class _mode:
    """Task split and split-precision mode for the length of a ``with``; afterwards the automatic split and the mode found before."""

    def __init__(self, tasks, sp=None):
        self.tasks, self.sp = tasks, sp

    def __enter__(self):
        from schnetpack_amd import _lib
        self.sp0 = _lib.get_split()
        if self.sp is not None:
            _lib.set_split(self.sp)
        _set_tasks(self.tasks)

    def __exit__(self, *exc):
        from schnetpack_amd import _lib
        _set_tasks(0)
        _lib.set_split(bool(self.sp0))


def _forces(m, batch, dev):
    """Forces of the two-launch potential; the molecule-resident backward must have run."""
    from schnetpack_amd import _lib, model as M
    _lib.profile_enable(True)
    _lib.profile_report()
    try:
        out = m(M.batch_to_inputs(batch, dev))
        f = out["forces"].detach().cpu()
        tags = set(_lib.profile_report())
    finally:
        _lib.profile_enable(False)
    assert {"schnet_mol_fwd", "schnet_mol_bwd"} <= tags and not any(t.startswith(("cfconv_", "pairwise")) for t in tags), tags
    return f


def _report(label, err, mol, bound, bad):
    print("%-58s worst molecule %4d  err %.3e  bound %.1e" % (label, mol, err, bound))
    if not err < bound:
        bad.append((label, mol, err, bound))


# ---------------------------------------------------------------------------------------------------------
# a. forces: every tile count, every split, every instance, workgroups that loop over unlike groups
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", [True, False])
@pytest.mark.parametrize("n_rbf", [8, 16, 20])
def test_forces_for_every_tile_count_and_task_split(dev, n_rbf, sp):
    from schnetpack_amd import _lib
    cus = _lib.device_info()["compute_units"]
    n_units = cus + 3 * len(CYCLE)
    units = tuple(CYCLE[k % len(CYCLE)] for k in range(n_units))
    assert cus % len(CYCLE) != 0, "a looping workgroup must meet an unlike group"
    b = _collate(units)
    ref = _reference(n_rbf)["forces"]
    rows = torch.cat([torch.arange(32 * (k % len(CYCLE)), 32 * (k % len(CYCLE)) + 32) for k in range(n_units)])
    ref = ref[rows]
    m = _model(n_rbf)
    got, bad = {}, []
    for tasks in (0, 1, 2):
        with _mode(tasks, sp):
            got[tasks] = _forces(m, b, dev)
        err, mol = C.per_molecule_err(got[tasks], ref, b["idx_m"])
        _report("n_rbf=%d split=%d tasks=%d vs float64" % (n_rbf, sp, tasks), err, mol, TOL, bad)
    for tasks in (0, 2):
        err, mol = C.per_molecule_err(got[tasks], got[1], b["idx_m"])
        _report("n_rbf=%d split=%d tasks=%d vs tasks=1" % (n_rbf, sp, tasks), err, mol, X_FORCES, bad)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# b. the representation-level call: dL/dx0 and dL/dR, and the `last` branch of the bottom interaction
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rep_reference(n_rbf, dtype=torch.float64):
    """Oracle of L = sum(x * G) with a seeded G: (G, dL/dx0 with the embedding rows as a leaf, dL/dR)."""
    b = _distinct_batch()
    p = {k: v.to(dtype) if v.is_floating_point() else v for k, v in _params(n_rbf)[0].items()}
    N = int(b["Z"].shape[0])
    x0 = p["embedding.weight"][b["Z"]].clone().requires_grad_(True)
    R = b["R"].to(dtype).clone().requires_grad_(True)
    q = dict(p)
    q["embedding.weight"] = x0
    r = O.pairwise_vectors(R, b["idx_i"], b["idx_j"], b["offsets"].to(dtype))
    x = O.schnet_representation(torch.arange(N), r, b["idx_i"], b["idx_j"], q, 3)
    G = torch.randn(N, 128, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    gx0, gR = torch.autograd.grad((x * G.to(dtype)).sum(), [x0, R])
    return G, gx0, gR


@pytest.mark.parametrize("sp", [True, False])
@pytest.mark.parametrize("n_rbf", [8, 16, 20])
def test_representation_gradients_with_and_without_dx0(dev, n_rbf, sp):
    from schnetpack_amd import _lib, model as M
    b = _distinct_batch()
    m = _model(n_rbf)
    rep = m.representation
    kind, p0, p1 = rep.radial_basis.kernel_params()
    G, gx0_ref, gR_ref = _rep_reference(n_rbf)
    Gd = G.float().to(dev)
    inp = M.batch_to_inputs(b, dev)
    bad = []
    for tasks in (0, 1, 2):
        for want_gx0 in (True, False):
            with _mode(tasks, sp):
                x0 = rep.embed(inp).detach().requires_grad_(want_gx0)
                R = inp["_positions"].detach().clone().requires_grad_(True)
                r = torch.ops.spk_hip.pairwise(R, inp["_idx_i"], inp["_idx_j"], inp["_offsets"])
                _lib.profile_enable(True)
                _lib.profile_report()
                try:
                    x = torch.ops.spk_hip.schnet(x0, r, inp["_idx_i"], inp["_idx_j"], rep.interaction_weights(), rep.n_filters, kind, p0, p1,
                                                 rep.cutoff_fn.cutoff_value())
                    grads = torch.autograd.grad((x * Gd).sum(), [R, x0] if want_gx0 else [R])
                    tags = set(_lib.profile_report())
                finally:
                    _lib.profile_enable(False)
            assert "schnet_mol_bwd" in tags, tags
            label = "n_rbf=%d split=%d tasks=%d dx0=%d" % (n_rbf, sp, tasks, want_gx0)
            err, mol = C.per_molecule_err(grads[0].cpu(), gR_ref, b["idx_m"])
            _report(label + " dL/dR vs float64", err, mol, TOL, bad)
            if want_gx0:
                err, mol = C.per_molecule_err(grads[1].cpu(), gx0_ref, b["idx_m"])
                _report(label + " dL/dx0 vs float64", err, mol, TOL, bad)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# c. a skin list: pairs beyond the cutoff are dropped from the tiles
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _skin_reference(name):
    rep, head = _params(20)
    return O.energy_and_forces("schnet", rep, head, C.batch(name), 3, dtype=torch.float64)


def test_skin_list_for_every_task_split(dev):
    bs, be = C.batch("skin384"), C.batch("skin384_exact")
    assert C.plan(bs)["meta"][5] == C.MAX_PAIRS and bs["idx_i"].shape[0] > be["idx_i"].shape[0]
    m = _model(20)
    bad = []
    for tasks in (0, 1, 2):
        with _mode(tasks):
            skin, exact = _forces(m, bs, dev), _forces(m, be, dev)
        assert torch.isfinite(skin).all()
        for label, got, ref, bound in (("skin list vs float64", skin, _skin_reference("skin384")["forces"], TOL),
                                       ("exact list vs float64", exact, _skin_reference("skin384_exact")["forces"], TOL),
                                       ("skin list vs exact list", skin, exact, X_FORCES)):
            err, mol = C.per_molecule_err(got, ref, bs["idx_m"])
            _report("skin384 tasks=%d %s" % (tasks, label), err, mol, bound, bad)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# d. reproducibility
# ---------------------------------------------------------------------------------------------------------
def test_one_task_per_tile_is_bit_reproducible(dev):
    """257 pairs: nine tiles, the last with one pair; 384: twelve.  One task per tile: every call returns the same bits.  Two tasks
    per tile add their partial sums in arrival order: equal to 1e-6 of max |F|, not compared bit for bit."""
    b = _collate((0, 257, 384, 257, 384, 0))
    m = _model(20)
    with _mode(1):
        first = _forces(m, b, dev)
        for k in range(9):
            assert torch.equal(_forces(m, b, dev), first), "call %d" % (k + 2)
    with _mode(2):
        two = _forces(m, b, dev)
    diff = float((two.double() - first.double()).abs().max() / first.double().abs().max())
    print("tasks=2 vs tasks=1: max |dF| / max |F| = %.3e  bound %.1e" % (diff, X_SPLIT))
    assert diff < X_SPLIT
