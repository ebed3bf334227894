"""The pair records of a group, handed from the molecule-resident SchNet forward to the backward through the records region of
``saved`` (csrc/spk_schnet_mol.hip: ``MolHandoff``; csrc/spk_schnet.hip: ``spk_schnet_mol_records_region``).

``spk_schnet_mol_set_bwd_records``: 0 = automatic (the region where there is one), 1 = the backward recomputes the records from the
list and the positions (the set-up before), 2 = the region is required.  The forward writes the same region in every mode, so 1
against 2 compares two set-ups of the backward on identical inputs: every output must be equal BIT FOR BIT -- forces / dL/dR of the
two-launch potential, dL/dr_ij and dL/dx0 of the representation operator -- for one and three interactions, both matrix paths and
n_rbf 8 and 20.

Groups (every unit is filled up to 32 atoms with single atoms, so the plan cannot merge across units; asserted on the host plan):
one atom, a dimer, 32 atoms x 384 pairs, 7 A lists of a 3.3 A cluster whose FIRST and LAST listed pair lie beyond the 5 A cutoff with
31, 32, 33, 64 and 65 pairs inside it, and -- between two full groups -- a group whose listed pairs are all beyond the cutoff.

The region exists where the caller asks for it (bit 1 of the model word beside bit 0): the operator library does, a caller that
sets bit 0 alone keeps the buffer size it had.  The C entry points with a caller-owned buffer show that the backward reads no word of
the region that the forward of the same call did not write (a buffer of quiet NaNs, a buffer used by a larger geometry before)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mol_capacity_cases as C
from oracle import spk_oracle as O
from schnetpack_amd import synthetic as S
from test_gpu_mol_fwd_operands import _CForward, _model as _biased_model

pytestmark = pytest.mark.gpu
COMBOS = [(L, sp, n_rbf) for L in (1, 3) for sp in (True, False) for n_rbf in (8, 20)]
INSIDE = (31, 32, 33, 64, 65)       # records inside the cutoff: one short of a tile, a tile, one over, two tiles, one over
QNAN = 0x7FC00000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------
def _fill(systems, first_seed):
    """The systems and single atoms up to exactly 32 atoms."""
    n = sum(len(s["Z"]) for s in systems)
    return list(systems) + [C.atom(first_seed + k) for k in range(C.MAX_ATOMS - n)]


def _inside(R, pi, pj):
    R32 = np.asarray(R, dtype=np.float32)
    return np.sqrt(((R32[pj] - R32[pi]) ** 2).sum(-1, dtype=np.float32)) < np.float32(C.CUTOFF)


@functools.lru_cache(maxsize=None)
def _skin_system(n_inside, seed):
    """A 16-atom cluster of 3.3 A radius with a 7 A list in canonical order whose first and last pair lie beyond 5 A, with exactly
    n_inside pairs inside 5 A between them and every pair beyond 5 A that lies between them.  Returns (system, pairs, pairs inside)."""
    Z, R = C.cluster(16, seed, radius=3.3)
    pi, pj = C._all_pairs(R, C.SKIN)
    assert np.array_equal(np.lexsort((pj, pi)), np.arange(pi.shape[0]))          # canonical order: the order of `half`
    ins = _inside(R, pi, pj)
    out = np.nonzero(~ins)[0]
    first, last = int(out[0]), int(out[-1])
    between = np.arange(first + 1, last)
    near = between[ins[between]]
    assert near.shape[0] >= n_inside, (seed, near.shape[0], n_inside)
    keep = np.sort(np.concatenate([[first], near[:n_inside], between[~ins[between]], [last]]))
    ins_k = ins[keep]
    assert not ins_k[0] and not ins_k[-1] and int(ins_k.sum()) == n_inside
    return C._system(Z, R, C._directed(pi[keep], pj[keep])), int(keep.shape[0]), n_inside


@functools.lru_cache(maxsize=None)
def _far_system():
    """Four atoms on a line, 5.5 A apart, with the three nearest-neighbour pairs of a 7 A list: no pair inside the cutoff."""
    R = np.array([[0.0, 0.0, 0.0], [5.5, 0.0, 0.0], [11.0, 0.0, 0.0], [16.5, 0.0, 0.0]])
    pi, pj = np.array([0, 1, 2]), np.array([1, 2, 3])
    assert not _inside(R, pi, pj).any()
    return C._system([6, 8, 1, 6], R, C._directed(pi, pj))


SKIN_SEEDS = {31: 1507, 32: 3233, 33: 2237, 64: 1507, 65: 3233}


@functools.lru_cache(maxsize=None)
def _edge_batch():
    """(batch, listed pairs per group, pairs inside the cutoff per group)."""
    full = C.capped(32, 384, 500)
    units = [([full], 384, 384), ([C.atom(950)], 0, 0), ([full], 384, 384), ([C.dimer(530)], 1, 1), ([full], 384, 384)]
    for n in INSIDE:
        s, listed, inside = _skin_system(n, SKIN_SEEDS[n])
        units.append((_fill([s], 1000 + 40 * n), listed, inside))
    units += [([full], 384, 384), (_fill([_far_system()], 3000), 3, 0), ([full], 384, 384)]
    b = S.collate([s for u in units for s in u[0]])
    plan = C.plan(b)
    assert np.diff(plan["grp_atom0"]).tolist() == [sum(len(s["Z"]) for s in u[0]) for u in units], "one group per unit"
    assert np.diff(plan["grp_pair0"]).tolist() == [u[1] for u in units], "listed pairs per group"
    e = plan["half"].astype(np.int64)
    R, ii, jj = b["R"].numpy(), b["idx_i"].numpy(), b["idx_j"].numpy()
    ins = _inside(R, ii[e], jj[e])
    got = [int(ins[p:q].sum()) for p, q in zip(plan["grp_pair0"][:-1], plan["grp_pair0"][1:])]
    assert got == [u[2] for u in units], "pairs inside the cutoff per group"
    return b, tuple(u[1] for u in units), tuple(u[2] for u in units)


@functools.lru_cache(maxsize=None)
def _loop_batch(n_groups):
    """dimer, 32 atoms x 384 pairs, dimer, ... : n_groups groups (odd), every dimer a group of its own."""
    systems = [C.dimer(530) if k % 2 == 0 else C.capped(32, 384, 500) for k in range(n_groups)]
    b = S.collate(systems)
    assert np.diff(C.plan(b)["grp_atom0"]).tolist() == [2 if k % 2 == 0 else 32 for k in range(n_groups)]
    return b


@functools.lru_cache(maxsize=None)
def _model(L, n_rbf):
    from schnetpack_amd import model as M
    rep, head = O.init_schnet_params(128, L, n_rbf, C.CUTOFF), O.init_atomwise_params(128, seed=1)
    m = M.build_model("schnet", 128, L, n_rbf, C.CUTOFF)
    M.load_reference_params(m, rep, head)
    return m.to(torch.device("cuda:0")).eval()


def _set_records(mode):
    from schnetpack_amd import _lib
    _lib.lib().spk_schnet_mol_set_bwd_records(ctypes.c_int(mode))


class _mode:
    """Records mode and matrix path for the length of a ``with``; afterwards the automatic mode and the path found before."""

    def __init__(self, records, sp=None):
        self.records, self.sp = records, sp

    def __enter__(self):
        from schnetpack_amd import _lib
        self.sp0 = _lib.get_split()
        if self.sp is not None:
            _lib.set_split(self.sp)
        _set_records(self.records)

    def __exit__(self, *exc):
        from schnetpack_amd import _lib
        _set_records(0)
        _lib.set_split(bool(self.sp0))


def _potential(m, batch, dev):
    """(energy, forces, tags) of the fused force call."""
    from schnetpack_amd import _lib, model as M
    _lib.profile_enable(True)
    _lib.profile_report()
    try:
        out = m(M.batch_to_inputs(batch, dev))
        res = out["energy"].detach().cpu(), out["forces"].detach().cpu()
        tags = set(_lib.profile_report())
    finally:
        _lib.profile_enable(False)
    return res[0], res[1], tags


def _representation(m, batch, dev):
    """(dL/dr_ij, dL/dx0, tags) of L = sum(x * G), seeded G, through the representation operator with r_ij given."""
    from schnetpack_amd import _lib, model as M
    rep = m.representation
    kind, p0, p1 = rep.radial_basis.kernel_params()
    inp = M.batch_to_inputs(batch, dev)
    x0 = rep.embed(inp).detach().requires_grad_(True)
    R = inp["_positions"].detach()
    r = (R[inp["_idx_j"]] - R[inp["_idx_i"]] + inp["_offsets"]).contiguous().requires_grad_(True)
    G = torch.randn(x0.shape, generator=torch.Generator().manual_seed(5)).to(dev)
    _lib.profile_enable(True)
    _lib.profile_report()
    try:
        x = torch.ops.spk_hip.schnet(x0, r, inp["_idx_i"], inp["_idx_j"], rep.interaction_weights(), rep.n_filters, kind, p0, p1,
                                     rep.cutoff_fn.cutoff_value())
        gr, gx0 = torch.autograd.grad((x * G).sum(), [r, x0])
        tags = set(_lib.profile_report())
    finally:
        _lib.profile_enable(False)
    return gr.cpu(), gx0.cpu(), tags


def _two_launches(tags):
    assert {"schnet_mol_fwd", "schnet_mol_bwd"} <= tags and not any(t.startswith(("cfconv_", "pairwise", "atomwise_")) for t in tags), tags


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------
# a. mode 1 against mode 2, bit for bit
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,sp,n_rbf", COMBOS)
def test_group_edges_recomputed_against_handed_over(dev, L, sp, n_rbf):
    b, listed, inside = _edge_batch()
    m = _model(L, n_rbf)
    res = {}
    for mode in (1, 2):
        with _mode(mode, sp):
            E, F, tags = _potential(m, b, dev)
            gr, gx0, tags_r = _representation(m, b, dev)
        _two_launches(tags)
        assert {"schnet_mol_fwd", "schnet_mol_bwd"} <= tags_r, tags_r
        res[mode] = (E, F, gr, gx0)
        for t in res[mode]:
            assert torch.isfinite(t).all()
    print("L=%d split=%d n_rbf=%d: listed %s inside %s; max |F| %.3e max |dL/dr| %.3e" % (L, sp, n_rbf, listed, inside,
          float(res[1][1].abs().max()), float(res[1][2].abs().max())))
    assert float(res[1][1].abs().max()) > 0 and float(res[1][2].abs().max()) > 0
    for name, x, y in zip(("energy", "forces", "dL/dr_ij", "dL/dx0"), res[1], res[2]):
        assert _same(x, y), (name, int((x != y).sum()))


@pytest.mark.parametrize("L,sp,n_rbf", COMBOS)
def test_grid_stride_loop_and_dimers_alone(dev, L, sp, n_rbf):
    """3 x CUs + 1 groups: every workgroup takes three or four groups, dimers and full groups in turn.  Mode 1 = mode 2, and every
    dimer has the forces of the dimer run as the first group of a three-group batch."""
    from schnetpack_amd import _lib
    n_groups = 3 * _lib.device_info()["compute_units"] + 1
    b = _loop_batch(n_groups)
    m = _model(L, n_rbf)
    res = {}
    for mode in (1, 2):
        with _mode(mode, sp):
            res[mode] = _potential(m, b, dev)
        _two_launches(res[mode][2])
    assert _same(res[1][0], res[2][0]) and _same(res[1][1], res[2][1])
    with _mode(2, sp):
        E1, F1, _ = _potential(m, S.collate([C.dimer(530), C.capped(32, 384, 500), C.aspirin(540)]), dev)
    start = np.concatenate([[0], np.cumsum([2 if k % 2 == 0 else 32 for k in range(n_groups)])])
    F = res[2][1]
    assert float(F1[:2].abs().max()) > 0
    for k in range(0, n_groups, 2):
        assert _same(F[start[k]:start[k] + 2], F1[:2]), "dimer of group %d" % k
        assert _same(res[2][0][k:k + 1], E1[:1]), "energy of the dimer of group %d" % k


@pytest.mark.parametrize("L,sp,n_rbf", COMBOS)
def test_periodic_offsets_through_the_potential(dev, L, sp, n_rbf):
    b = S.periodic_molecule_batch("aspirin", 6, seed=4)
    assert (b["offsets"] != 0).any()
    m = _model(L, n_rbf)
    res = {}
    for mode in (1, 2):
        with _mode(mode, sp):
            res[mode] = _potential(m, b, dev)
        _two_launches(res[mode][2])
    assert float(res[1][1].abs().max()) > 0
    assert _same(res[1][0], res[2][0]) and _same(res[1][1], res[2][1])


def test_two_calls_are_bit_equal_and_launch_the_two_kernels(dev):
    """Automatic mode: the profile tags of the fused call are exactly the two launches, and a second call returns the same bits."""
    m = _model(3, 20)
    for b in (S.molecule_batch("aspirin", 8, seed=2), _edge_batch()[0]):
        with _mode(0):
            E1, F1, tags = _potential(m, b, dev)
            E2, F2, _ = _potential(m, b, dev)
        assert tags == {"schnet_mol_fwd", "schnet_mol_bwd"}, tags
        assert _same(E1, E2) and _same(F1, F2)


# ---------------------------------------------------------------------------------------------------------
# b. every head width behind both set-ups
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["ssp", "silu"])
@pytest.mark.parametrize("H", [32, 64, 96, 128])
def test_head_widths_against_float64_with_both_setups(dev, H, act):
    """Part 2 of the head's gradient (waves 0-3) runs beside the per-edge records (waves 4-7) behind the records' barrier.  Head widths
    32 ... 128 with both activations, split path, biases that are not zero, groups of 1, 2, 21, 27 and 32 atoms (the batch, models and
    float64 oracle of tests/test_gpu_mol_head_setup.py): energies and forces within 1e-5, and the two set-ups agree bit for bit."""
    from conftest import rel_err
    import test_gpu_mol_head_setup as HS
    b = HS._occupancy_batch()
    e_ref, f_ref = HS._head_reference(3, H, act)
    m = HS._head_model(3, H, act)
    got = {}
    for mode in (1, 2):
        with _mode(mode, True):
            got[mode] = HS._potential(m, b, dev)
    err_e, err_f = rel_err(got[2][0], e_ref), rel_err(got[2][1], f_ref)
    print("H=%d %s split: rel err energy %.3e forces %.3e  bound 1e-5" % (H, act, err_e, err_f))
    assert err_e <= 1e-5 and err_f <= 1e-5
    assert _same(got[1][0], got[2][0]) and _same(got[1][1], got[2][1])


# ---------------------------------------------------------------------------------------------------------
# c. the C entry points with a caller-owned `saved`
# ---------------------------------------------------------------------------------------------------------
class _Driver(_CForward):
    """spk_schnet_forward_f32 + spk_schnet_backward_f32 on one caller-owned ``saved``; records=True sets bit 1 of the model word before
    the buffer is sized."""

    def __init__(self, m, batch, dev, records=True):
        super().__init__(m, batch, dev)
        self.dev = dev
        self.n_saved_plain = self.n_saved
        if records:
            self.m.reserved = 3
            self.n_saved = int(self.lib.spk_schnet_saved_floats_graph(ctypes.byref(self.m), self.plan.graph(), ctypes.byref(self.rb)))
        self.gx = torch.randn(self.N, 128, generator=torch.Generator().manual_seed(9)).to(dev)

    def buffer(self, bits=None):
        saved = torch.zeros(self.n_saved, dtype=torch.float32, device=self.dev)
        if bits is not None:
            saved.view(torch.int32).fill_(bits)
        return saved

    def forward(self, saved, r_ij=None):
        _lib = self._lib
        out = torch.zeros(self.N, 128, dtype=torch.float32, device=self.dev)
        r = self.r_ij if r_ij is None else r_ij
        _lib.check(self.lib.spk_schnet_forward_f32(ctypes.byref(self.m), self.plan.graph(), ctypes.byref(self.rb), _lib.fptr(self.x0), _lib.fptr(r),
                                                   _lib.fptr(out), _lib.fptr(saved), _lib.fptr(self.scratch), _lib.stream()))
        return out

    def backward_rc(self, saved, r_ij=None):
        _lib = self._lib
        r = self.r_ij if r_ij is None else r_ij
        gr = torch.full((int(r.shape[0]), 3), float("nan"), dtype=torch.float32, device=self.dev)
        gx0 = torch.full((self.N, 128), float("nan"), dtype=torch.float32, device=self.dev)
        _lib.profile_enable(True)
        _lib.profile_report()
        try:
            rc = self.lib.spk_schnet_backward_f32(ctypes.byref(self.m), self.plan.graph(), ctypes.byref(self.rb), _lib.fptr(self.gx), _lib.fptr(r),
                                                  _lib.fptr(saved), _lib.fptr(self.scratch), _lib.fptr(gr), _lib.fptr(gx0), _lib.stream())
            torch.cuda.synchronize()
            tags = set(_lib.profile_report())
        finally:
            _lib.profile_enable(False)
        return rc, gr.cpu(), gx0.cpu(), tags

    def run(self, saved, r_ij=None):
        x = self.forward(saved, r_ij).cpu()
        rc, gr, gx0, tags = self.backward_rc(saved, r_ij)
        self._lib.check(rc)
        assert "schnet_mol_bwd" in tags, tags
        return x, gr, gx0


@pytest.mark.parametrize("sp", [True, False])
def test_poisoned_saved_buffer(dev, sp):
    """All of ``saved`` holds quiet NaNs before the forward: the backward reads nothing the forward did not write -- records beyond the
    count of a group, map entries and vectors beyond its list, groups without a record."""
    b, _, _ = _edge_batch()
    with _mode(2, sp):
        drv = _Driver(_biased_model(20, "gaussian", biased=True), b, dev)
        clean = drv.run(drv.buffer())
        poisoned = drv.run(drv.buffer(QNAN))
    for name, x, y in zip(("x", "dL/dr_ij", "dL/dx0"), clean, poisoned):
        assert torch.isfinite(y).all(), name
        assert _same(x, y), name
    assert float(clean[1].abs().max()) > 0


def test_reused_saved_buffer(dev):
    """Two geometries of one list through one buffer, the second stretched by 1.25 (fewer pairs inside the cutoff, one group left with
    none): equal to the second geometry in a fresh buffer."""
    b, _, _ = _edge_batch()
    with _mode(2, True):
        drv = _Driver(_biased_model(20, "gaussian", biased=True), b, dev)
        r2 = (1.25 * drv.r_ij).contiguous()
        d1, d2 = drv.r_ij.norm(dim=1), r2.norm(dim=1)
        assert int((d2 < C.CUTOFF).sum()) < int((d1 < C.CUTOFF).sum())
        saved = drv.buffer()
        first = drv.run(saved)
        second = drv.run(saved, r2)
        fresh = drv.run(drv.buffer(), r2)
    for name, x, y in zip(("x", "dL/dr_ij", "dL/dx0"), second, fresh):
        assert torch.isfinite(x).all() and _same(x, y), name
    assert not _same(first[1], second[1])


def test_required_region_that_is_not_there_is_an_error(dev):
    """Mode 2 and a buffer sized without bit 1 of the model word: the library's error, no launch."""
    from schnetpack_amd import _lib
    b, _, _ = _edge_batch()
    drv = _Driver(_biased_model(20, "gaussian", biased=True), b, dev, records=False)
    saved = drv.buffer()
    drv.forward(saved)
    with _mode(2):
        rc, _, _, tags = drv.backward_rc(saved)
        msg = _lib.lib().spk_last_error()
    assert rc != 0 and b"records" in msg, (rc, msg)
    assert not any("_bwd" in t for t in tags), tags
    with _mode(0):                                   # automatic: the recomputing set-up
        rc, gr, gx0, tags = drv.backward_rc(saved)
    assert rc == 0 and "schnet_mol_bwd" in tags and torch.isfinite(gr).all() and torch.isfinite(gx0).all()
    # and the same numbers as with the region
    with _mode(2):
        drv2 = _Driver(_biased_model(20, "gaussian", biased=True), b, dev)
        _, gr2, gx02 = drv2.run(drv2.buffer())
    assert _same(gr, gr2) and _same(gx0, gx02)


def test_sizing(dev):
    """With bit 1 the buffer of an eligible list grows by exactly spk_schnet_mol_records_floats() = 8 n_half + n_groups + the padding to
    a multiple of four; without it, and for a model the molecule-resident backward does not cover (n_rbf = 32), it is the sum of the
    regions it had: L x N x 256 + L x filter rows (+ the per-call pair list, absent on these lists)."""
    b, _, _ = _edge_batch()
    drv = _Driver(_biased_model(20, "gaussian", biased=True), b, dev)
    lib = drv.lib
    n_half, n_groups = drv.n_half, int(drv.grp_atom0.shape[0]) - 1
    plain = drv.L * drv.N * 256 + drv.L * (-(-n_half // 32) * 32 * 128)
    assert drv.n_saved_plain == plain
    rec = int(lib.spk_schnet_mol_records_floats(ctypes.byref(drv.m), drv.plan.graph(), ctypes.byref(drv.rb)))
    pad = (-plain) % 4
    print("n_half %d groups %d: plain %d records %d (padding %d)" % (n_half, n_groups, plain, rec, pad))
    assert rec == pad + 8 * n_half + n_groups and drv.n_saved == plain + rec
    d = _Driver(_biased_model(32, "gaussian", biased=True), b, dev)
    assert d.m.reserved == 3
    assert int(lib.spk_schnet_mol_records_floats(ctypes.byref(d.m), d.plan.graph(), ctypes.byref(d.rb))) == 0
    assert d.n_saved == d.n_saved_plain == plain
