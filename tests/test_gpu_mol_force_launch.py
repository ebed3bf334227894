"""The SchNet molecule force call in ONE launch (csrc/spk_schnet_mol.hip: ``k_schnet_mol_force`` -- forward and backward of every group in
the same workgroup, back to back) against the two launches ``k_schnet_mol_fwd`` + ``k_schnet_mol_bwd``.

``spk_schnet_mol_set_force_launches``: 0 = automatic (one launch where the call is eligible and the per-launch profile is off),
1 = one launch also under the profile (tag ``schnet_mol_force``; an error where the call is not eligible), 2 = always two launches.
Every case runs with the switch at 1 and at 2 and compares the two with each other -- energies bit for bit, forces to 1e-6 of the
largest force: the one launch runs the two launches' instructions on the same data, and the per-pair sums of the backward meet in LDS
in task order, so two runs agree as closely as that and not necessarily bit for bit -- and each with the float64 oracle
(oracle/spk_oracle.py), to the project's bound of 1e-5 per molecule.  "Alone" and "twice" comparisons are bit for bit.

Groups, models and references are those of tests/test_gpu_mol_matrix_overlap.py, test_gpu_mol_stagger.py and test_gpu_mol_head_setup.py
(helpers imported, caches shared).  n_rbf = 32 (four k-blocks) is a forward-only shape of the molecule-resident kernels -- the backward's
LDS footprint ends at three k-blocks -- so that model runs the stage-by-stage path with either switch, which the case asserts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mol_capacity_cases as C
import test_gpu_mol_head_setup as HS
import test_gpu_mol_matrix_overlap as T
from oracle import spk_oracle as O
from schnetpack_amd import synthetic as S
from test_gpu_mol_fwd_operands import _CForward, _model as _biased_model, _params as _biased_params

pytestmark = pytest.mark.gpu
TOL = 1e-5             # against the float64 oracle
TOL_MODES = 1e-6       # forces of the one-launch call against the two-launch call
FORCE, TWO = {"schnet_mol_force"}, {"schnet_mol_fwd", "schnet_mol_bwd"}
EDGE_PAIRS = (1, 32, 33, 161, 384)
QNAN = 0x7FC00000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _set_launches(mode):
    from schnetpack_amd import _lib
    _lib.lib().spk_schnet_mol_set_force_launches(ctypes.c_int(mode))


class _launches:
    """Launch switch (and matrix path, records mode) for the length of a ``with``; afterwards automatic / what was found before."""

    def __init__(self, mode, sp=None, records=0):
        self.mode, self.sp, self.records = mode, sp, records

    def __enter__(self):
        from schnetpack_amd import _lib
        self.sp0 = _lib.get_split()
        if self.sp is not None:
            _lib.set_split(self.sp)
        _lib.lib().spk_schnet_mol_set_bwd_records(ctypes.c_int(self.records))
        _set_launches(self.mode)

    def __exit__(self, *exc):
        from schnetpack_amd import _lib
        _set_launches(0)
        _lib.lib().spk_schnet_mol_set_bwd_records(ctypes.c_int(0))
        _lib.set_split(bool(self.sp0))


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _both(label, m, b, dev):
    """The force call with the switch at 1 and at 2: tags, energies bit-equal, forces within TOL_MODES.  Returns the two results."""
    with _launches(1):
        E1, F1, t1 = T._potential(m, b, dev)
    with _launches(2):
        E2, F2, t2 = T._potential(m, b, dev)
    assert t1 == FORCE and t2 == TWO, (t1, t2)
    assert torch.isfinite(E1).all() and torch.isfinite(F1).all() and torch.isfinite(F2).all(), label
    df = _rel(F1, F2) if float(F2.abs().max()) > 0 else float(F1.abs().max())
    print("%-44s one launch against two: energies bit-equal %s, forces %.3e  bound %.0e" % (label, T._same(E1, E2), df, TOL_MODES))
    assert T._same(E1, E2), label
    assert df <= TOL_MODES, (label, df)
    return (E1, F1), (E2, F2)


# ---------------------------------------------------------------------------------------------------------
# a. tile and capacity edges, model shapes
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_batch():
    b = S.collate([C.capped(32, P, 600 + P) for P in EDGE_PAIRS])
    T._one_group_per_unit(b, [32] * len(EDGE_PAIRS), EDGE_PAIRS)
    return b


@functools.lru_cache(maxsize=None)
def _edge_reference(L, n_rbf):
    rep, head = T._params(L, n_rbf)
    return O.energy_and_forces("schnet", rep, head, _edge_batch(), L, dtype=torch.float64)


@pytest.mark.parametrize("n_rbf", [8, 16, 20])
@pytest.mark.parametrize("L", [1, 3])
def test_pair_tile_edges_one_launch_against_two(dev, L, n_rbf):
    """32-atom groups of 1, 32, 33, 161 and 384 pairs; one and three interactions; one, two and three k-blocks of the radial basis."""
    b, m = _edge_batch(), T._model(L, n_rbf)
    one, two = _both("tile edges L=%d n_rbf=%d" % (L, n_rbf), m, b, dev)
    assert float(one[1][:32].abs().max()) > 0, "the one-pair group has forces"
    for lab, (E, F) in (("one", one), ("two", two)):
        T._check("tile edges L=%d n_rbf=%d, %s" % (L, n_rbf, lab), E, F, _edge_reference(L, n_rbf), b["idx_m"])


def test_four_k_blocks_are_not_a_shape_of_the_backward(dev):
    """n_rbf = 32: the molecule-resident backward does not cover it, so the force call is not the fused potential and the switch does
    not apply -- neither value raises, neither runs k_schnet_mol_force, and the results are the oracle's."""
    b, m = _edge_batch(), T._model(3, 32)
    res = {}
    for mode in (1, 2):
        with _launches(mode):
            res[mode] = T._potential(m, b, dev)
        assert "schnet_mol_force" not in res[mode][2] and "schnet_mol_bwd" not in res[mode][2], res[mode][2]
        T._check("n_rbf=32, switch %d" % mode, res[mode][0], res[mode][1], _edge_reference(3, 32), b["idx_m"])
    assert T._same(res[1][0], res[2][0])


@pytest.mark.parametrize("L", [1, 3])
def test_small_groups_and_a_group_without_pairs(dev, L):
    """32 | 1 | 32 | 2 | 32 atoms, a group whose listed pairs all lie beyond the cutoff, 32: forces of the empty group exactly zero, its
    neighbours bit for bit what they are alone."""
    units, b, m = T._group_edge_units(), T._group_edge_batch(), T._model(L, 20)
    start = T._group_start(units)
    one, two = _both("group edges L=%d" % L, m, b, dev)
    mol0 = [sum(len(u) for u in units[:k]) for k in range(len(units))]
    for lab, mode, (E, F) in (("one", 1, one), ("two", 2, two)):
        T._check("group edges L=%d, %s" % (L, lab), E, F, T._reference("group_edges", L, 20), b["idx_m"])
        assert int((F[start[5]:start[6]] != 0).sum()) == 0, "no pair inside the cutoff: no force"
        assert int((F[start[1]:start[2]] != 0).sum()) == 0, "a single atom: no force"
        assert float(F[start[3]:start[4]].abs().max()) > 0, "the dimer has forces"
        for k in (4, 6):
            with _launches(mode):
                E1, F1, _ = T._potential(m, S.collate(list(units[k])), dev)
            assert float(F1.abs().max()) > 0
            assert T._same(F[start[k]:start[k + 1]], F1), "forces of group %d beside the empty group (%s)" % (k, lab)
            assert T._same(E[mol0[k]:mol0[k] + 1], E1), "energy of group %d beside the empty group (%s)" % (k, lab)


@pytest.mark.parametrize("act", ["ssp", "silu"])
@pytest.mark.parametrize("H", [32, 128])
@pytest.mark.parametrize("L", [1, 3])
def test_head_widths_and_activations(dev, L, H, act):
    """Head widths 32 and 128 (one and four row tiles), shifted softplus and SiLU, head biases that are not zero, on groups of 1, 2, 21,
    27 and 32 atoms."""
    from conftest import rel_err
    b = HS._occupancy_batch()
    e_ref, f_ref = HS._head_reference(L, H, act)
    one, two = _both("head H=%d %s L=%d" % (H, act, L), HS._head_model(L, H, act), b, dev)
    for lab, (E, F) in (("one", one), ("two", two)):
        err_e, err_f = rel_err(E, e_ref), rel_err(F, f_ref)
        print("H=%d %s L=%d, %s: rel err energy %.3e forces %.3e  bound %.0e" % (H, act, L, lab, err_e, err_f, TOL))
        assert err_e <= TOL and err_f <= TOL


def test_filter_network_biases_not_zero(dev):
    b = _edge_batch()
    rep, head = _biased_params(20, "gaussian", True)
    ref = O.energy_and_forces("schnet", rep, head, b, 3, dtype=torch.float64)
    one, two = _both("biased filter network", _biased_model(20, "gaussian", biased=True), b, dev)
    for lab, (E, F) in (("one", one), ("two", two)):
        T._check("biased filter network, %s" % lab, E, F, ref, b["idx_m"])


def test_aspirin_with_skin_lists(dev):
    """Two aspirin frames with 7 A lists: the pair compaction is on."""
    b = T._skin_aspirin_batch()
    one, two = _both("aspirin 7 A lists", T._model(3, 20), b, dev)
    for lab, (E, F) in (("one", one), ("two", two)):
        T._check("aspirin 7 A lists, %s" % lab, E, F, T._reference("skin_aspirin", 3, 20), b["idx_m"])


# ---------------------------------------------------------------------------------------------------------
# b. the loop over the groups: a workgroup runs the forward of ALL its groups, then their backward, in the same LDS
# ---------------------------------------------------------------------------------------------------------
def test_group_loop_dimers_as_alone_and_two_calls_bit_equal(dev):
    """3 x CUs + 1 groups, dimers and 384-pair groups in turn: every dimer has the bits of the dimer alone, a second call the bits of
    the first, with either switch."""
    from schnetpack_amd import _lib
    n_groups = 3 * _lib.device_info()["compute_units"] + 1
    b, m = T._loop_batch(n_groups), T._model(3, 20)
    one, two = _both("group loop, %d groups" % n_groups, m, b, dev)
    start = np.concatenate([[0], np.cumsum([2 if k % 2 == 0 else 32 for k in range(n_groups)])])
    for lab, mode, (E, F) in (("one", 1, one), ("two", 2, two)):
        with _launches(mode):
            E2, F2, _ = T._potential(m, b, dev)
            E1, F1, _ = T._potential(m, S.collate([C.dimer(530)]), dev)
        assert float(F1.abs().max()) > 0
        assert T._same(E, E2) and T._same(F, F2), "two consecutive calls differ (%s)" % lab
        bad = [k for k in range(0, n_groups, 2) if not (T._same(F[start[k]:start[k] + 2], F1) and T._same(E[k:k + 1], E1))]
        assert not bad, "dimers that differ from the dimer alone (%s): groups %s" % (lab, bad[:8])
        assert all(T._same(F[start[k]:start[k + 1]], F[start[1]:start[2]]) for k in range(3, n_groups, 2)), "full groups differ (%s)" % lab


# ---------------------------------------------------------------------------------------------------------
# c. the C entry points: energy routes, edge gradient, caller-owned `saved`, graph capture
# ---------------------------------------------------------------------------------------------------------
class _Forces(_CForward):
    """spk_schnet_potential_forces_f32 / _forces_gr_f32 on a collated batch with a caller-owned ``saved`` (records region included)."""

    def __init__(self, m, batch, dev):
        from schnetpack_amd import _lib, model as M
        super().__init__(m, batch, dev)
        self.dev = dev
        self.m.reserved = 3
        self.n_saved = int(self.lib.spk_schnet_saved_floats_graph(ctypes.byref(self.m), self.plan.graph(), ctypes.byref(self.rb)))
        inp = M.batch_to_inputs(batch, dev)
        self.R = inp["_positions"].detach().float().contiguous()
        self.off = inp["_offsets"].detach().float().contiguous()
        self.idx_m = inp["_idx_m"].contiguous()
        self.n_mol = int(batch["n_mol"])
        l0, l1 = m.output_modules[0].outnet[0], m.output_modules[0].outnet[1]
        hw = [l0.weight.detach().float().contiguous(), l0.weight.detach().float().t().contiguous(), l0.bias.detach().float().contiguous(),
              l1.weight.detach().float().contiguous(), l1.bias.detach().float().contiguous()]
        self.keep.append(hw)
        self.H = int(hw[0].shape[0])
        self.head = _lib.HeadT(*[w.data_ptr() for w in hw], self.H, int(m.output_modules[0]._head_act))
        assert self.lib.spk_schnet_potential_supported(ctypes.byref(self.m), ctypes.byref(self.head), self.plan.graph(), ctypes.byref(self.rb)) == 1
        self.n_edges = int(self.idx_i.shape[0])

    def buffer(self, bits=None):
        saved = torch.zeros(self.n_saved, dtype=torch.float32, device=self.dev)
        if bits is not None:
            saved.view(torch.int32).fill_(bits)
        return saved

    def outputs(self):
        nan = float("nan")
        mk = lambda *shape: torch.full(shape, nan, dtype=torch.float32, device=self.dev)
        return {"x": mk(self.N, 128), "E": mk(self.n_mol), "F": mk(self.N, 3), "gr": mk(self.n_edges, 3), "pre_h": mk(self.N, self.H)}

    def launch(self, o, saved, R=None, inside=1, gr=False):
        """Enqueue the call on the current stream; returns the library's status."""
        _lib, f = self._lib, self._lib.fptr
        R = self.R if R is None else R
        args = [ctypes.byref(self.m), ctypes.byref(self.head), self.plan.graph(), ctypes.byref(self.rb), f(self.x0), None, None, 0, f(R), f(self.off),
                _lib.iptr(self.idx_m), self.n_mol, inside, f(o["x"]), f(o["E"]), f(o["F"])]
        if gr:
            return self.lib.spk_schnet_potential_forces_gr_f32(*args, f(o["gr"]), f(o["pre_h"]), f(saved), _lib.stream())
        return self.lib.spk_schnet_potential_forces_f32(*args, f(o["pre_h"]), f(saved), _lib.stream())

    def run(self, mode, saved=None, R=None, inside=1, gr=False, sp=True, records=0, prof=True):
        """(outputs on the host, tags) with the switch at `mode`."""
        _lib = self._lib
        o = self.outputs()
        if not inside:
            o["E"].zero_()                       # (the atomic route accumulates; the library clears E itself -- this only removes the NaN)
        with _launches(mode, sp, records):
            _lib.profile_enable(prof)
            _lib.profile_report()
            try:
                _lib.check(self.launch(o, self.buffer() if saved is None else saved, R, inside, gr))
                torch.cuda.synchronize()
                tags = set(_lib.profile_report())
            finally:
                _lib.profile_enable(False)
        return {k: v.cpu() for k, v in o.items()}, tags


def test_three_molecules_in_one_group_on_the_store_and_the_atomic_route(dev):
    b = S.collate([C.ethanol(521), C.ethanol(522), C.ethanol(523)])
    assert np.diff(C.plan(b)["grp_atom0"]).tolist() == [27] and int(b["n_mol"]) == 3
    rep, head = T._params(3, 20)
    ref = O.energy_and_forces("schnet", rep, head, b, 3, dtype=torch.float64)
    drv = _Forces(T._model(3, 20), b, dev)
    for route, inside in (("store", 1), ("atomic", 0)):
        o1, t1 = drv.run(1, inside=inside)
        o2, t2 = drv.run(2, inside=inside)
        assert t1 == FORCE and TWO <= t2 and "schnet_mol_force" not in t2, (t1, t2)
        df = _rel(o1["F"], o2["F"])
        print("%-6s route: energies %s, one launch against two: forces %.3e" % (route, o1["E"].tolist(), df))
        assert T._same(o1["E"], o2["E"]) and df <= TOL_MODES
        for lab, o in (("one", o1), ("two", o2)):
            T._check("three ethanol frames, %s route, %s" % (route, lab), o["E"], o["F"], ref, b["idx_m"])


def test_edge_gradient_route(dev):
    """spk_schnet_potential_forces_gr_f32: dE/dr of every edge and the forces, one launch against two; the forces of the _gr call are
    those of the plain call bit for bit, as the header promises."""
    b = _edge_batch()
    drv = _Forces(T._model(3, 20), b, dev)
    o1, t1 = drv.run(1, gr=True)
    o2, t2 = drv.run(2, gr=True)
    p1, _ = drv.run(1)
    assert t1 == FORCE and t2 == TWO, (t1, t2)
    assert torch.isfinite(o1["gr"]).all() and float(o2["gr"].abs().max()) > 0
    dg, df = _rel(o1["gr"], o2["gr"]), _rel(o1["F"], o2["F"])
    print("edge gradient: one launch against two: dE/dr %.3e forces %.3e  bound %.0e" % (dg, df, TOL_MODES))
    assert T._same(o1["E"], o2["E"]) and dg <= TOL_MODES and df <= TOL_MODES
    assert T._same(o1["E"], p1["E"]) and _rel(o1["F"], p1["F"]) <= TOL_MODES
    T._check("edge gradient route, one launch", o1["E"], o1["F"], _edge_reference(3, 20), b["idx_m"])


def test_caller_owned_saved_poisoned_and_reused(dev):
    """``saved`` full of quiet NaNs, and a buffer a larger geometry used before: the backward half reads nothing that the forward half
    of the same call did not write -- the outputs are those of a clean buffer, bit for bit."""
    b = T._group_edge_batch()
    drv = _Forces(T._model(3, 20), b, dev)
    for mode in (1, 2):
        clean, _ = drv.run(mode)
        poisoned, _ = drv.run(mode, saved=drv.buffer(QNAN))
        R2 = (1.25 * drv.R).contiguous()                 # stretched: fewer pairs inside the cutoff
        saved = drv.buffer()
        first, _ = drv.run(mode, saved=saved)
        second, _ = drv.run(mode, saved=saved, R=R2)
        fresh, _ = drv.run(mode, R=R2)
        for k in ("E", "F", "x", "pre_h"):
            assert torch.isfinite(poisoned[k]).all(), (mode, k)
            assert T._same(clean[k], poisoned[k]), "switch %d: %s with a poisoned buffer" % (mode, k)
            assert T._same(second[k], fresh[k]), "switch %d: %s with a reused buffer" % (mode, k)
        assert not T._same(first["F"], second["F"])


def test_graph_capture_and_three_replays(dev):
    """The one-launch call captured in a HIP graph (profile off: the automatic rule picks it) and replayed three times equals the
    eager call."""
    b = _edge_batch()
    drv = _Forces(T._model(3, 20), b, dev)
    eager, tags = drv.run(1)
    assert tags == FORCE
    o, saved = drv.outputs(), drv.buffer()
    with _launches(0, True):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            drv._lib.check(drv.launch(o, saved))             # warm-up outside the capture (attribute set-up, first launch)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rc = drv.launch(o, saved)
        drv._lib.check(rc)
        for rep in range(3):
            for v in o.values():
                v.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            for k in ("E", "F", "x"):
                assert T._same(o[k].cpu(), eager[k]) if k != "F" else _rel(o[k].cpu(), eager[k]) <= TOL_MODES, (rep, k)


# ---------------------------------------------------------------------------------------------------------
# d. which route runs
# ---------------------------------------------------------------------------------------------------------
def test_route_selection(dev):
    from schnetpack_amd import _lib
    b = S.molecule_batch("aspirin", 4, seed=3)
    drv = _Forces(T._model(3, 20), b, dev)
    ref, tags = drv.run(0)
    assert tags == TWO, "automatic with the profile on keeps the two launches: %s" % tags
    _, tags = drv.run(1)
    assert tags == FORCE, tags
    _, tags = drv.run(2)
    assert tags == TWO, tags
    off, tags = drv.run(0, prof=False)           # automatic, profile off: the one launch -- no tag to read, the results are the check
    assert tags == set() and T._same(off["E"], ref["E"]) and _rel(off["F"], ref["F"]) <= TOL_MODES
    _, tags = drv.run(0, sp=False)
    assert tags == TWO, tags
    _, tags = drv.run(0, records=1)
    assert tags == TWO, tags
    for kw in ({"sp": False}, {"records": 1}):       # switch 1 on a call that is not eligible: the library's error, no launch
        with pytest.raises(_lib.SpkHipError, match="eligible"):
            drv.run(1, **kw)
    _, tags = drv.run(2)                           # (and the switch is back where it was)
    assert tags == TWO
