"""Operands of the molecule-resident SchNet forward (csrc/spk_schnet_mol.hip) on the pair-tile edges of tests/mol_fwd_operand_cases.py:
the radial basis comes from a table staged per launch (padding slots k >= n_rbf hold benign values and meet zero columns of W1), and
the modulation loop is branch-free -- a padding row of the last tile takes the record of the tile's last pair and stores that pair's
filter row again.

Against the float64 oracle the bound is the project's 1e-5, per MOLECULE (max|got - ref| / max|ref| over the atoms of one molecule);
between two device paths 2e-6 on the representation and 5e-6 on the forces, as in tests/test_gpu_mol.py.  The saved filter outputs
are reached through the C entry ``spk_schnet_forward_f32`` with a caller-owned ``saved`` buffer (layout: L x (h | pre3), then per
interaction the raw filter outputs, row = position of the pair in ``half``).  Every figure is printed before it is asserted."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mol_capacity_cases as C
import mol_fwd_operand_cases as F
from conftest import rel_err
from oracle import spk_oracle as O
from schnetpack_amd import synthetic as S

pytestmark = pytest.mark.gpu
TOL = 1e-5
X_REP, X_FORCES = 2e-6, 5e-6
BASES = [(8, "gaussian"), (16, "gaussian"), (20, "gaussian"), (32, "gaussian"), (13, "gaussian"),
         (8, "bessel"), (16, "bessel"), (20, "bessel"), (32, "bessel"), (13, "bessel")]
SENTINEL = -float(2 ** 33)          # exact in float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _split:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from schnetpack_amd import _lib
        self.before = _lib.get_split()
        _lib.set_split(self.on)

    def __exit__(self, *exc):
        from schnetpack_amd import _lib
        _lib.set_split(bool(self.before))


@functools.lru_cache(maxsize=None)
def _params(n_rbf, radial, biased=False):
    rep, head = O.init_schnet_params(128, 3, n_rbf, F.CUTOFF, radial=radial), O.init_atomwise_params(128, seed=1)
    if biased:                      # the seeded init has zero biases: give the filter network some
        gen = torch.Generator().manual_seed(5)
        for l in range(3):
            for k in (0, 1):
                rep["interactions.%d.filter_network.%d.bias" % (l, k)] = 0.2 * torch.randn(128, generator=gen)
    return rep, head


def _model(n_rbf, radial, biased=False):
    from schnetpack_amd import model as M
    rep, head = _params(n_rbf, radial, biased)
    m = M.build_model("schnet", 128, 3, n_rbf, F.CUTOFF, radial)
    M.load_reference_params(m, rep, head)
    return m.to(torch.device("cuda:0")).eval()


def _run(m, batch, dev, general=False):
    from schnetpack_amd import _lib, model as M
    _lib.set_variant(_lib.VARIANT_MFMA_DIRECTED if general else _lib.VARIANT_AUTO)
    try:
        _lib.profile_enable(True)
        _lib.profile_report()
        inp = M.batch_to_inputs(batch, dev)
        out = m(inp)
        res = {"energy": out["energy"].detach().cpu(), "forces": out["forces"].detach().cpu(),
               "scalar_representation": inp["scalar_representation"].detach().cpu()}
        tags = set(_lib.profile_report())
    finally:
        _lib.profile_enable(False)
        _lib.set_variant(_lib.VARIANT_AUTO)
    return res, tags


@functools.lru_cache(maxsize=None)
def _distinct_reference(n_rbf, radial):
    """float64 oracle of every distinct system (computed once per basis; never modified)."""
    rep, head = _params(n_rbf, radial)
    return O.energy_and_forces("schnet", rep, head, F.distinct_batch(), 3, dtype=torch.float64, need_rep=True)


def _oracle_errors(label, got, ref, idx_m, names):
    bad = []
    for key in ("forces", "scalar_representation", "energy"):
        err, mol = C.energy_err(got[key], ref[key]) if key == "energy" else C.per_molecule_err(got[key], ref[key], idx_m)
        print("%-40s %-22s worst molecule %5d (%s)  err %.3e  bound %.1e" % (label, key, mol, names[mol], err, TOL))
        if not err < TOL:
            bad.append((label, key, names[mol], err))
    return bad


# ---------------------------------------------------------------------------------------------------------
# a. parity on every case, every KPB instance, both bases, both matrix paths
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("n_rbf,radial", BASES)
def test_parity_on_the_tile_edges(dev, n_rbf, radial, split):
    """Every case of mol_fwd_operand_cases in one batch of >= 3 groups per workgroup (a workgroup meets unlike groups one after the
    other): representation, energy and forces per molecule against the float64 oracle, and against the general driver."""
    from schnetpack_amd import _lib
    cycles = F.loop_cycles(_lib.device_info()["compute_units"])
    b, names = F.batch(cycles), F.labels(cycles)
    ref = F.expand(_distinct_reference(n_rbf, radial), cycles)
    m = _model(n_rbf, radial)
    with _split(split):
        got, tags = _run(m, b, dev)
        gen, tags_gen = _run(m, b, dev, general=True)
    assert "schnet_mol_fwd" in tags and not any(t.startswith("cfconv_fwd") for t in tags), tags
    assert ("schnet_mol_bwd" in tags) == (n_rbf <= 24), tags
    assert not any("_mol_" in t for t in tags_gen), tags_gen
    bad = _oracle_errors("n_rbf=%d %s split=%d" % (n_rbf, radial, split), got, ref, b["idx_m"], names)
    bad += _oracle_errors("n_rbf=%d %s split=%d general" % (n_rbf, radial, split), gen, ref, b["idx_m"], names)
    ex, ef = rel_err(got["scalar_representation"], gen["scalar_representation"]), rel_err(got["forces"], gen["forces"])
    print("molecule path vs general driver: representation %.3e (bound %.1e)  forces %.3e (bound %.1e)" % (ex, X_REP, ef, X_FORCES))
    assert not bad, bad
    assert ex < X_REP and ef < X_FORCES


# ---------------------------------------------------------------------------------------------------------
# b. the saved filter outputs, through the C entry with a caller-owned buffer
# ---------------------------------------------------------------------------------------------------------
class _CForward:
    """spk_schnet_forward_f32 on a collated batch with the filters saved (``reserved`` bit 0), as the operator library calls it."""

    def __init__(self, m, batch, dev):
        from schnetpack_amd import _lib, model as M, ops
        self.lib, self._lib = _lib.lib(), _lib
        rep = m.representation
        inp = M.batch_to_inputs(batch, dev)
        R = inp["_positions"]
        self.idx_i, self.idx_j = inp["_idx_i"], inp["_idx_j"]
        self.r_ij = (R[self.idx_j] - R[self.idx_i] + inp["_offsets"]).contiguous()
        self.x0 = rep.embedding(inp["_atomic_numbers"]).detach().contiguous()
        self.N = int(self.x0.shape[0])
        self.plan = ops.EdgePlan(self.idx_i, self.idx_j, self.N, self.r_ij)
        ws = [w.detach().float().contiguous() for w in rep.interaction_weights()]
        self.L = len(ws) // 9
        self.keep = [ws]
        layers = (_lib.SchnetLayerT * self.L)()
        for l in range(self.L):
            t = ws[9 * l:9 * l + 9]
            tr = [t[0].t().contiguous(), t[5].t().contiguous(), t[7].t().contiguous()]
            self.keep.append(tr)
            for name, w in zip(("in2f_w", "fn_w1", "fn_b1", "fn_w2", "fn_b2", "f2out_w1", "f2out_b1", "f2out_w2", "f2out_b2",
                                "in2f_wT", "f2out_w1T", "f2out_w2T"), t + tr):
                setattr(layers[l], name, w.data_ptr())
        self.layers = layers
        self.m = _lib.SchnetT(128, 128, self.L, 1, layers, None)
        n_pack = int(self.lib.spk_schnet_packed_floats(ctypes.byref(self.m)))
        assert n_pack > 0
        self.wpack = torch.empty(n_pack, dtype=torch.float32, device=dev)
        _lib.check(self.lib.spk_schnet_pack_weights_f32(ctypes.byref(self.m), _lib.fptr(self.wpack), _lib.stream()))
        self.m.wpack = self.wpack.data_ptr()
        kind, p0, p1 = rep.radial_basis.kernel_params()
        self.p = (p0.detach().float().contiguous(), None if p1 is None else p1.detach().float().contiguous())
        self.rb = _lib.RadialT(kind, int(self.p[0].shape[0]), _lib.fptr(self.p[0]), _lib.fptr(self.p[1]), rep.cutoff_fn.cutoff_value())
        self.n_saved = int(self.lib.spk_schnet_saved_floats_graph(ctypes.byref(self.m), self.plan.graph(), ctypes.byref(self.rb)))
        self.n_half = int(self.plan.half.shape[0])
        self.gsz = (self.n_saved - self.L * self.N * 256) // self.L
        assert self.gsz >= self.n_half * 128
        self.scratch = torch.empty(int(self.lib.spk_schnet_scratch_floats(ctypes.byref(self.m), self.N)), dtype=torch.float32, device=dev)
        self.grp_atom0, self.grp_pair0 = self.plan.groups[0].cpu().numpy(), self.plan.groups[1].cpu().numpy()

    def __call__(self, groups=None):
        """One launch (over the groups [g0, g1) of the plan only, if given) into buffers filled with a sentinel; returns
        (x_out, saved, tags)."""
        _lib = self._lib
        out = torch.full((self.N, 128), SENTINEL, dtype=torch.float32, device=self.x0.device)
        saved = torch.full((self.n_saved,), SENTINEL, dtype=torch.float32, device=self.x0.device)
        g = type(self.plan._graph).from_buffer_copy(self.plan._graph)
        if groups is not None:
            g0, g1 = groups
            g.n_groups = g1 - g0
            g.grp_atom0 = self.plan.groups[0].data_ptr() + 4 * g0
            g.grp_pair0 = self.plan.groups[1].data_ptr() + 4 * g0
        _lib.profile_enable(True)
        _lib.profile_report()
        try:
            _lib.check(self.lib.spk_schnet_forward_f32(ctypes.byref(self.m), ctypes.byref(g), ctypes.byref(self.rb), _lib.fptr(self.x0), _lib.fptr(self.r_ij),
                                                       _lib.fptr(out), _lib.fptr(saved), _lib.fptr(self.scratch), _lib.stream()))
            torch.cuda.synchronize()
            tags = set(_lib.profile_report())
        finally:
            _lib.profile_enable(False)
        return out.cpu(), saved.cpu(), tags

    def filter_rows(self, saved):
        """[L, n_half, 128] view of the raw filter outputs in a host copy of ``saved``."""
        base = self.L * self.N * 256
        return torch.stack([saved[base + l * self.gsz: base + l * self.gsz + self.n_half * 128].view(self.n_half, 128) for l in range(self.L)])

    def pair_edges(self):
        return self.plan.half.cpu().long()


def _filter_oracle(rep, d, n_layers=3):
    """float64 W2 ssp(W1 phi + b1) + b2 of every distance, per interaction: [L, P, 128]."""
    p = {k: v.double() if v.is_floating_point() else v for k, v in rep.items()}
    phi = O._radial(d, p)
    rows = []
    for l in range(n_layers):
        pre = "interactions.%d.filter_network." % l
        rows.append(O.dense(O.dense(phi, p[pre + "0.weight"], p[pre + "0.bias"], O.shifted_softplus), p[pre + "1.weight"], p[pre + "1.bias"]))
    return torch.stack(rows)


@pytest.mark.parametrize("n_rbf,radial,split", [(20, "gaussian", True), (20, "gaussian", False), (8, "gaussian", True), (13, "bessel", True),
                                                 (16, "gaussian", True), (32, "gaussian", True)])
def test_saved_filter_rows_of_the_ragged_cases(dev, n_rbf, radial, split):
    """One cycle of the cases (22 groups).  (i) the row of every pair inside the cutoff is the oracle's filter row -- also the last pair
    of a ragged tile, which the padding rows store again; (ii) a launch over the groups [6, 15) leaves every byte outside their rows
    at the sentinel; (iii) two launches give bit-equal buffers."""
    b = F.batch(1)
    m = _model(n_rbf, radial, biased=True)
    rep, _ = _params(n_rbf, radial, biased=True)
    with _split(split):
        fwd = _CForward(m, b, dev)
        x1, s1, tags = fwd()
        x2, s2, _ = fwd()
        xs, ss, tags_s = fwd(groups=(6, 15))
    assert "schnet_mol_fwd" in tags and "schnet_mol_fwd" in tags_s, (tags, tags_s)
    assert torch.equal(s1, s2) and torch.equal(x1, x2)                                   # (iii)
    # (i)
    e = fwd.pair_edges()
    r32 = fwd.r_ij.cpu()[e].double()                                                      # the float32 pair vectors the device sees
    d = torch.sqrt((r32 * r32).sum(1))
    inside = d < F.CUTOFF
    ref, got = _filter_oracle(rep, d), fwd.filter_rows(s1).double()
    scale = ref[:, inside].abs().amax(dim=(1, 2), keepdim=True)
    err = ((got - ref).abs() / scale)[:, inside]
    pair_group = np.searchsorted(fwd.grp_pair0, np.arange(fwd.n_half), side="right") - 1
    worst = int(err.amax(dim=(0, 2)).argmax())
    print("n_rbf=%d %s split=%d: %d of %d rows inside the cutoff, worst row error %.3e (group %s)"
          % (n_rbf, radial, split, int(inside.sum()), fwd.n_half, float(err.max()), F.CYCLE[pair_group[np.nonzero(inside.numpy())[0][worst]]]))
    assert torch.isfinite(got[:, inside]).all() and float(err.max()) < TOL
    for g, label in enumerate(F.CYCLE):                                                   # the last pair inside the cutoff of every group: the row the padding repeats
        rows = np.nonzero((pair_group == g) & inside.numpy())[0]
        if rows.size:
            assert float(((got[:, rows[-1]] - ref[:, rows[-1]]).abs() / scale[:, 0]).max()) < TOL, label
    # rows of pairs beyond the cutoff: never read by the molecule-resident backward (it compacts the same way); when they are written
    # they hold the filter row too
    out_err = ((got - ref).abs() / scale)[:, ~inside]
    untouched = (got[:, ~inside] == SENTINEL).all(dim=2)
    assert (untouched | (out_err.amax(dim=2) < TOL)).all()
    # (ii)
    a0, a1 = int(fwd.grp_atom0[6]), int(fwd.grp_atom0[15])
    q0, q1 = int(fwd.grp_pair0[6]), int(fwd.grp_pair0[15])
    assert (xs[:a0] == SENTINEL).all() and (xs[a1:] == SENTINEL).all() and torch.equal(xs[a0:a1], x1[a0:a1])
    hp = ss[:fwd.L * fwd.N * 256].view(fwd.L, 2, fwd.N, 128)
    assert (hp[:, :, :a0] == SENTINEL).all() and (hp[:, :, a1:] == SENTINEL).all()
    assert torch.equal(hp[:, :, a0:a1], s1[:fwd.L * fwd.N * 256].view(fwd.L, 2, fwd.N, 128)[:, :, a0:a1])
    gs, g1 = fwd.filter_rows(ss), fwd.filter_rows(s1)
    assert (gs[:, :q0] == SENTINEL).all() and (gs[:, q1:] == SENTINEL).all() and torch.equal(gs[:, q0:q1], g1[:, q0:q1])
    tail = fwd.L * fwd.N * 256
    for l in range(fwd.L):
        assert (ss[tail + l * fwd.gsz + fwd.n_half * 128: tail + (l + 1) * fwd.gsz] == SENTINEL).all()


def _prefix_system(P):
    """The 12-atom cluster of the cases with the first P of its 66 pairs in canonical (i, j) order: atom 0 pairs with every atom, so
    the system is one block for every P >= 11, and P -> P + 1 appends a pair BEHIND the last one."""
    Z, R = C.cluster(12, 930)
    pi, pj = C._all_pairs(R, F.CUTOFF)
    order = np.lexsort((pj, pi))[:P]
    return C._system(Z, R, C._directed(pi[order], pj[order]))


@pytest.mark.parametrize("n_rbf,radial", [(8, "gaussian"), (16, "gaussian"), (20, "gaussian"), (32, "gaussian"), (13, "gaussian"), (16, "bessel")])
def test_padding_rows_repeat_the_last_pair_bit_for_bit(dev, n_rbf, radial):
    """The unconditional store of the branch-free modulation loop writes, for every padding row, the row of the tile's last pair to that
    pair's address.  That is harmless only if the value is the SAME: with P pairs the last pair's row is stored by its own row and by
    32 - P % 32 padding rows; with P + 1 pairs (one appended behind it) it is the second to last and stored once.  The filter row of a
    pair depends on its distance alone, so all P rows must be bit-equal between the two groups -- P = 31 ... 33 and 63 ... 65, against
    P + 1 (P + 1 = 32, 64: a full tile, no padding at all)."""
    counts = (31, 32, 33, 34, 63, 64, 65, 66)
    systems = []
    for P in counts:
        systems += [_prefix_system(P), F.system("aspirin")]
    b = S.collate(systems)
    with _split(True):
        fwd = _CForward(_model(n_rbf, radial, biased=True), b, dev)
        _, saved, tags = fwd()
    assert "schnet_mol_fwd" in tags, tags
    assert np.diff(fwd.grp_atom0).tolist() == [12, 21] * len(counts) and np.diff(fwd.grp_pair0)[::2].tolist() == list(counts)
    rows = fwd.filter_rows(saved)
    assert torch.isfinite(rows).all()
    for k, P in enumerate(counts[:-1]):
        if counts[k + 1] != P + 1:
            continue
        q0, q1 = int(fwd.grp_pair0[2 * k]), int(fwd.grp_pair0[2 * k + 2])
        same = torch.equal(rows[:, q0:q0 + P], rows[:, q1:q1 + P])
        print("n_rbf=%d %s: %d pairs against %d: rows bit-equal %s" % (n_rbf, radial, P, P + 1, same))
        assert same, (P, (rows[:, q0:q0 + P] != rows[:, q1:q1 + P]).any(dim=(0, 2)).nonzero().flatten().tolist())


# ---------------------------------------------------------------------------------------------------------
# c. the basis table is made on every launch
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radial", ["gaussian", "bessel"])
def test_basis_parameters_changed_between_two_calls(dev, radial):
    """Offsets and widths (Bessel: frequencies) of ONE model scaled in place between two calls: each call equals the oracle with the
    parameters of that call, and the two differ by far more than the bound."""
    b, names = F.batch(1), F.labels(1)
    m = _model(20, radial)
    rep, head = _params(20, radial)
    rep = dict(rep)
    res = []
    for scale_o, scale_w in ((1.0, 1.0), (0.93, 1.21)):
        with torch.no_grad():
            if radial == "gaussian":
                m.representation.radial_basis.offsets.mul_(scale_o)
                m.representation.radial_basis.widths.mul_(scale_w)
                rep["radial_basis.offsets"], rep["radial_basis.widths"] = rep["radial_basis.offsets"] * scale_o, rep["radial_basis.widths"] * scale_w
            else:
                m.representation.radial_basis.freqs.mul_(scale_o)
                rep["radial_basis.freqs"] = rep["radial_basis.freqs"] * scale_o
        got, tags = _run(m, b, dev)
        assert "schnet_mol_fwd" in tags, tags
        dist = O.energy_and_forces("schnet", rep, head, F.distinct_batch(), 3, dtype=torch.float64, need_rep=True)
        bad = _oracle_errors("%s scaled %.2f / %.2f" % (radial, scale_o, scale_w), got, F.expand(dist, 1), b["idx_m"], names)
        assert not bad, bad
        res.append(got)
    moved = rel_err(res[1]["scalar_representation"], res[0]["scalar_representation"])
    print("%s: representation moved by %.3e between the calls" % (radial, moved))
    assert moved > 100 * TOL
