"""The general-list SchNet kernels (csrc/spk_cfconv.hip) on the row and tile edges of tests/cfconv_box_cases.py: the row-tile forward
(forced through ``spk_cfconv_set_rowtile``), the pair forward on both matrix paths, the saved-filter pair backward with and without
dL/dh, the per-call compaction of skin lists and both XCD-contiguous walks -- none of them through the molecule-resident kernels
(plans without groups; asserted by profile tag).

Bounds.  Against the float64 formula the project's 1e-5, measured twice: max|got - ref| / max|ref| over the tensor, and per row
max_c |got - ref| / max_c sum_e |W_e o h_j| (the row's own sum of absolute contributions, from the reference); saved filter rows per
pair against the row's max|ref|.  Between two device paths 2e-6 on outputs and 5e-6 on gradients (tests/test_gpu_mol.py).  Rows
without a pair inside the cutoff and dL/dr of pairs at or beyond it are exactly 0; the row-tile forward is bit-reproducible.  Every
figure is printed before it is asserted; the worst per case and kernel are recorded in profiles/cfconv_box_edges.md."""
import ctypes

import numpy as np
import pytest
import torch

import cfconv_box_cases as B

pytestmark = pytest.mark.gpu
TOL = 1e-5
X_OUT, X_GRAD = 2e-6, 5e-6
SENTINEL = -float(2 ** 33)          # exact in float32
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _mode:
    """Row-tile switch and matrix path for the calls inside; both restored on exit."""

    def __init__(self, rowtile, split):
        self.rowtile, self.split = rowtile, split

    def __enter__(self):
        from schnetpack_amd import _lib
        self.before = _lib.get_split()
        _lib.set_split(self.split)
        _lib.lib().spk_cfconv_set_rowtile(self.rowtile)

    def __exit__(self, *exc):
        from schnetpack_amd import _lib
        _lib.set_split(bool(self.before))
        _lib.lib().spk_cfconv_set_rowtile(0)


def _profiled(fn):
    """Run fn() with the launch profile on: (result, {tag: count}) of the cfconv kernels; no molecule-resident kernel may appear."""
    from schnetpack_amd import _lib
    _lib.profile_enable(True)
    _lib.profile_report()
    try:
        res = fn()
        torch.cuda.synchronize()
        rep = _lib.profile_report()
    finally:
        _lib.profile_enable(False)
    assert not any("_mol" in t for t in rep), rep
    return res, {t: c[0] for t, c in rep.items() if t.startswith("cfconv")}


def _radial(n_rbf, radial, dev):
    from schnetpack_amd import _lib, ops
    ps = [p.float().contiguous().to(dev) for p in B.radial_params(n_rbf, radial)]
    kind = _lib.SPK_RBF_GAUSSIAN if radial == "gaussian" else _lib.SPK_RBF_BESSEL
    return ops.radial_struct(kind, n_rbf, ps[0], ps[1] if len(ps) > 1 else None, B.CUTOFF), ps


def _plan(c, dev, filtered=False, transposed=False):
    from schnetpack_amd import ops
    plan = ops.EdgePlan(c["idx_i"].to(dev), c["idx_j"].to(dev), c["N"], c["r_ij"].to(dev), want_groups=False)
    assert plan.sorted and plan.groups is None
    if transposed:
        plan.build_transposed()
    if filtered:
        plan.set_filter(True)
    return plan


def _report(label, what, figs, bound):
    print("%-44s %-8s %s  (bound %.1e)" % (label, what, "  ".join("%s %.3e" % kv for kv in figs.items()), bound))
    return [(label, what, k, v) for k, v in figs.items() if not v < bound]


# ---------------------------------------------------------------------------------------------------------
# a. operator level
# ---------------------------------------------------------------------------------------------------------
class _Op:
    """spk_schnet_cfconv_fwd_f32 / _bwd_f32 on a case, outputs into NaN-filled buffers (gr is accumulated into: it starts at 0)."""

    def __init__(self, c, n_rbf, radial, dev, transposed=False):
        self.c, self.dev = c, dev
        self.plan = _plan(c, dev, transposed=transposed)
        self.rb, self.keep = _radial(n_rbf, radial, dev)
        self.p = B.filter_params(n_rbf)
        self.w = [self.p[k].contiguous().to(dev) for k in ("w1", "b1", "w2", "b2")]
        h, gy = B.features(c["N"], 11)
        self.h, self.gy = h, gy
        self.hd, self.gyd, self.rd = h.to(dev), gy.to(dev), c["r_ij"].contiguous().to(dev)

    def fwd(self):
        from schnetpack_amd import _lib
        y = torch.full((self.c["N"], B.NF), NAN, device=self.dev)
        f = _lib.fptr
        _lib.check(_lib.lib().spk_schnet_cfconv_fwd_f32(self.plan.graph(), ctypes.byref(self.rb), f(self.hd), f(self.rd), f(self.w[0]), f(self.w[1]),
                                                        f(self.w[2]), f(self.w[3]), B.NF, f(y), _lib.stream()))
        return y

    def bwd(self):
        from schnetpack_amd import _lib
        gh = torch.full((self.c["N"], B.NF), NAN, device=self.dev)
        gr = torch.zeros(len(self.c["idx_i"]), 3, device=self.dev)
        f = _lib.fptr
        _lib.check(_lib.lib().spk_schnet_cfconv_bwd_f32(self.plan.graph(), ctypes.byref(self.rb), f(self.hd), f(self.gyd), f(self.rd), f(self.w[0]), f(self.w[1]),
                                                        f(self.w[2]), f(self.w[3]), B.NF, f(gh), f(gr), _lib.stream()))
        return gh, gr


FWD_MODES = (("rowtile", 1, True), ("pair_split", -1, True), ("rowtile_asked_fp32", 1, False), ("pair_fp32", -1, False))


def _check_rows(label, what, got, ref, scale):
    assert torch.isfinite(got).all(), (label, what, "unwritten or non-finite rows", (~torch.isfinite(got)).any(1).nonzero().flatten()[:8].tolist())
    fig, row, dead = B.per_row_err(got, ref, scale)
    assert not dead, (label, what, "rows without a pair inside the cutoff are not exactly 0", dead[:8])
    return _report(label, "%s (worst row %d)" % (what, row), {"max-norm": B.max_norm_err(got, ref), "per-row": fig}, TOL)


def _operator_case(c, n_rbf, radial, dev, symmetric):
    label = "%s n_rbf=%d %s" % (c["info"]["name"], n_rbf, radial)
    op = _Op(c, n_rbf, radial, dev, transposed=not symmetric)
    assert op.plan.symmetric == symmetric
    ref = B.cfconv_ref(c, op.h, op.p, radial, gy=op.gy)
    lengths = torch.from_numpy(B.row_lengths(c))
    beyond = torch.from_numpy(B.d32(c) >= np.float32(B.CUTOFF))
    bad, ys, grads = [], {}, {}
    for name, rowtile, split in FWD_MODES:
        with _mode(rowtile, split):
            y, tags = _profiled(op.fwd)
            want = "cfconv_fwd_rowtile" if (rowtile > 0 and split) else ("cfconv_fwd_pair" if symmetric else "cfconv_fwd_mfma")
            assert tags == {want: 1}, (label, name, tags)
            if want == "cfconv_fwd_rowtile":
                assert torch.equal(y, op.fwd()), (label, "the row-tile forward is not bit-reproducible")
            y = y.cpu()
            assert (y[lengths == 0] == 0).all(), (label, name, "empty rows")
            bad += _check_rows(label + " " + name, "y", y, ref["y"], ref["scale_y"])
            ys[name] = y
            if symmetric and rowtile > 0:
                continue                    # the backward of a symmetric list does not depend on the row-tile switch
            (gh, gr), tags = _profiled(op.bwd)
            if symmetric:
                assert tags == {"cfconv_bwd_pair": 1}, (label, name, tags)
            else:                            # by-neighbour pass = the forward kernel over the transposed list, then the directed backward without the scatter
                assert tags == {want: 1, "cfconv_bwd_mfma_atomic": 1}, (label, name, tags)
            gh, gr = gh.cpu(), gr.cpu()
            by_j = torch.from_numpy(B.row_lengths(c, "idx_j"))
            assert (gh[by_j == 0] == 0).all(), (label, name, "empty by-neighbour rows")
            assert (gr[beyond] == 0).all(), (label, name, "dL/dr of pairs at or beyond the cutoff")
            bad += _check_rows(label + " " + name, "gh", gh, ref["gh"], ref["scale_gh"])
            bad += _report(label + " " + name, "gr", {"max-norm": B.max_norm_err(gr, ref["gr"])}, TOL)
            grads[name] = (gh, gr)
    # between device paths
    for a, b in (("rowtile", "pair_split"), ("pair_split", "pair_fp32"), ("rowtile_asked_fp32", "pair_fp32")):
        bad += _report(label, "%s vs %s" % (a, b), {"y": B.max_norm_err(ys[a], ys[b])}, X_OUT)
    names = sorted(grads)
    for a, b in zip(names, names[1:]):
        bad += _report(label, "%s vs %s" % (a, b), {"gh": B.max_norm_err(grads[a][0], grads[b][0]), "gr": B.max_norm_err(grads[a][1], grads[b][1])}, X_GRAD)
    assert not bad, bad


@pytest.mark.parametrize("n_rbf,radial", B.BASES)
@pytest.mark.parametrize("name", ["rows_last1", "rows_last32", "cutoff"])
def test_operator_on_the_row_edges(dev, name, n_rbf, radial):
    """Rows of 0, 1, 31 ... 97 pairs (and rows with pairs on both sides of the cutoff, one pair exactly at it): y from the row-tile forward
    and from the pair forward on both matrix paths, gh and gr from the recomputing pair backward (one instance, run with the split switch on and
    off; the split backward is the saved-filter one of the driver tests below), against float64 per tensor and per row."""
    c = {"rows_last1": lambda: B.rows(1), "rows_last32": lambda: B.rows(32), "cutoff": B.cutoff}[name]()
    _operator_case(c, n_rbf, radial, dev, symmetric=True)


@pytest.mark.parametrize("n_rbf,radial", B.BASES)
def test_operator_on_an_asymmetric_list(dev, n_rbf, radial):
    """Sorted asymmetric list with its by-neighbour copy: two row-tile launches (rows, by-neighbour rows of 0 ... 150 pairs) plus the directed
    backward; with the switch off or on the fp32 path the directed forward kernel twice."""
    _operator_case(B.asymmetric(), n_rbf, radial, dev, symmetric=False)


def test_operator_on_the_xcd_walks(dev):
    """A ring list sized for the device so that the row-tile forward walks the atoms and the pair kernels walk the tiles XCD-contiguously, with a
    ragged last eighth in both."""
    from schnetpack_amd import _lib
    cus = _lib.device_info()["compute_units"]
    c = B.walk(cus)
    cond = c["info"]
    print(cond)
    assert cond["n_at_least_2_14"] and cond["n_not_multiple_of_8"] and cond["tiles_at_least_16_per_workgroup"] and cond["tiles_not_multiple_of_8"]
    assert cond["pair_walk_live"] and cond["row_walk_live"], (cus, cond)
    _operator_case(c, 20, "gaussian", dev, symmetric=True)


# ---------------------------------------------------------------------------------------------------------
# b. driver level: saved filters, compaction, saved-filter backward
# ---------------------------------------------------------------------------------------------------------
class _Driver:
    """spk_schnet_forward_f32 / spk_schnet_backward_f32 with a caller-owned ``saved`` buffer and ``reserved`` bit 0 (filters saved), as the
    operator library calls them.  saved = L x (h | pre3) | L x filter rows [gsz] | (filtered lists) compacted pair list, count."""

    def __init__(self, c, n_rbf, radial, n_layers, dev, filtered=False):
        from schnetpack_amd import _lib
        self.c, self.dev, self.L, self._lib, self.lib = c, dev, n_layers, _lib, _lib.lib()
        self.rep = B.model_params(n_rbf, radial, n_layers)
        self.plan = _plan(c, dev, filtered=filtered)
        assert self.plan.symmetric
        self.filtered = filtered
        self.N, self.E = c["N"], len(c["idx_i"])
        self.rd = c["r_ij"].contiguous().to(dev)
        self.x0, self.gx_out = B.features(self.N, 12)
        self.x0d, self.gxd = self.x0.to(dev), self.gx_out.to(dev)
        D = lambda t: t.float().contiguous().to(dev)
        self.keep = []
        layers = (_lib.SchnetLayerT * n_layers)()
        for l in range(n_layers):
            pre = "interactions.%d." % l
            t = {"in2f_w": self.rep[pre + "in2f.weight"], "fn_w1": self.rep[pre + "filter_network.0.weight"], "fn_b1": self.rep[pre + "filter_network.0.bias"],
                 "fn_w2": self.rep[pre + "filter_network.1.weight"], "fn_b2": self.rep[pre + "filter_network.1.bias"],
                 "f2out_w1": self.rep[pre + "f2out.0.weight"], "f2out_b1": self.rep[pre + "f2out.0.bias"],
                 "f2out_w2": self.rep[pre + "f2out.1.weight"], "f2out_b2": self.rep[pre + "f2out.1.bias"]}
            t.update({"in2f_wT": t["in2f_w"].t(), "f2out_w1T": t["f2out_w1"].t(), "f2out_w2T": t["f2out_w2"].t()})
            for name, w in t.items():
                wd = D(w)
                self.keep.append(wd)
                setattr(layers[l], name, wd.data_ptr())
        self.layers = layers
        self.m = _lib.SchnetT(B.NF, B.NF, n_layers, 1, layers, None)
        n_pack = int(self.lib.spk_schnet_packed_floats(ctypes.byref(self.m)))
        assert n_pack > 0
        self.wpack = torch.empty(n_pack, dtype=torch.float32, device=dev)
        _lib.check(self.lib.spk_schnet_pack_weights_f32(ctypes.byref(self.m), _lib.fptr(self.wpack), _lib.stream()))
        self.m.wpack = self.wpack.data_ptr()
        self.rb, self.rkeep = _radial(n_rbf, radial, dev)
        self.n_saved = int(self.lib.spk_schnet_saved_floats_graph(ctypes.byref(self.m), self.plan.graph(), ctypes.byref(self.rb)))
        self.n_half = int(self.plan.half.shape[0])
        self.base = self.L * self.N * 2 * B.NF
        self.gsz = -(-self.n_half // B.TILE) * B.TILE * B.NF
        assert self.n_saved >= self.base + self.L * self.gsz + (self.n_half + 4 if filtered else 0)
        self.scratch = torch.empty(int(self.lib.spk_schnet_scratch_floats(ctypes.byref(self.m), self.N)), dtype=torch.float32, device=dev)

    def forward(self):
        _lib = self._lib
        out = torch.full((self.N, B.NF), SENTINEL, dtype=torch.float32, device=self.dev)
        saved = torch.full((self.n_saved,), SENTINEL, dtype=torch.float32, device=self.dev)
        _lib.check(self.lib.spk_schnet_forward_f32(ctypes.byref(self.m), self.plan.graph(), ctypes.byref(self.rb), _lib.fptr(self.x0d), _lib.fptr(self.rd),
                                                   _lib.fptr(out), _lib.fptr(saved), _lib.fptr(self.scratch), _lib.stream()))
        return out, saved

    def backward(self, saved, want_gx0):
        _lib = self._lib
        gr = torch.full((self.E, 3), NAN, dtype=torch.float32, device=self.dev)      # the driver assigns or clears it itself
        gx0 = torch.full((self.N, B.NF), NAN, dtype=torch.float32, device=self.dev) if want_gx0 else None
        _lib.check(self.lib.spk_schnet_backward_f32(ctypes.byref(self.m), self.plan.graph(), ctypes.byref(self.rb), _lib.fptr(self.gxd), _lib.fptr(self.rd),
                                                    _lib.fptr(saved), _lib.fptr(self.scratch), _lib.fptr(gr), _lib.fptr(gx0), _lib.stream()))
        return gr, gx0

    def filter_area(self, saved_host, l):
        return saved_host[self.base + l * self.gsz: self.base + (l + 1) * self.gsz].view(-1, B.NF)

    def compacted(self, saved_host):
        """(list, count) the forward wrote behind the filters."""
        words = saved_host[self.base + self.L * self.gsz: self.base + self.L * self.gsz + self.n_half + 4].view(torch.int32)
        return words[:self.n_half], int(words[self.n_half])


def _filter_reference(drv, radial, edges):
    """float64 raw filter rows [L, P, 128] of the float32 distances of `edges`."""
    d = torch.from_numpy(B.d32(drv.c)[edges])
    rows = []
    for l in range(drv.L):
        pre = "interactions.%d.filter_network." % l
        p = {"n_rbf": int(drv.rb.n_rbf), "w1": drv.rep[pre + "0.weight"], "b1": drv.rep[pre + "0.bias"], "w2": drv.rep[pre + "1.weight"], "b2": drv.rep[pre + "1.bias"]}
        rows.append(B.filter_rows(d, p, radial))
    return torch.stack(rows)


DRIVER_FWD = (("rowtile", 1, True), ("pair_split", -1, True), ("pair_fp32", -1, False))


def _driver_case(c, n_rbf, radial, n_layers, dev, filtered):
    label = "%s%s n_rbf=%d %s L=%d" % (c["info"]["name"], " filtered" if filtered else "", n_rbf, radial, n_layers)
    drv = _Driver(c, n_rbf, radial, n_layers, dev, filtered)
    L = n_layers
    ref = B.representation_ref(c, drv.x0, drv.rep, L, radial, gx_out=drv.gx_out)
    half = B.canonical(c)
    assert np.array_equal(drv.plan.half.cpu().numpy(), half)
    live = B.live_pairs(c)
    rows_of = live if filtered else half                       # the pair whose filter row is row k of the filter area
    inside = torch.from_numpy(B.d32(c)[rows_of] < np.float32(B.CUTOFF))
    fref = _filter_reference(drv, radial, rows_of)
    beyond = torch.from_numpy(B.d32(c) >= np.float32(B.CUTOFF))
    P = len(rows_of)
    bad, res = [], {}
    for name, rowtile, split in DRIVER_FWD:
        with _mode(rowtile, split):
            (x, saved), tags = _profiled(drv.forward)
        rowtile_ran = rowtile > 0 and not filtered               # saving through edge_pair needs the plan's own pair list
        assert tags == {"cfconv_fwd_rowtile" if rowtile_ran else "cfconv_fwd_pair": L}, (label, name, tags)
        x, sh = x.cpu(), saved.cpu()
        assert torch.isfinite(sh[:drv.base]).all() and (sh[:drv.base] != SENTINEL).all(), (label, name, "h | pre3")
        bad += _report(label + " " + name, "x_out", {"max-norm": B.max_norm_err(x, ref["x_out"])}, TOL)
        if filtered:
            act, count = drv.compacted(sh)
            assert count == len(live) and np.array_equal(act[:count].numpy(), live), (label, name, "compacted list", count, len(live))
        for l in range(L):
            area = drv.filter_area(sh, l)
            got = area[:P].double()
            if P:
                assert torch.isfinite(got).all() and (got != SENTINEL).all(), (label, name, l, "unwritten filter rows",
                                                                               (got == SENTINEL).any(1).nonzero().flatten()[:8].tolist())
                err = ((got - fref[l]).abs().amax(1) / fref[l].abs().amax(1))[inside]
                if err.numel():
                    worst = int(err.argmax())
                    bad += _report(label + " " + name, "filter rows l=%d (worst: row %d)" % (l, int(inside.nonzero().flatten()[worst])), {"per-pair": float(err.max())}, TOL)
            written_to = P if rowtile_ran else -(-P // B.TILE) * B.TILE          # the pair kernels store the padding rows of the last tile
            assert (area[written_to:] == SENTINEL).all(), (label, name, l, "rows of no pair were written",
                                                           (area[written_to:] != SENTINEL).any(1).nonzero().flatten()[:8].tolist())
        out = {"x": x}
        for bsplit in (True, False):
            with _mode(rowtile, bsplit):
                (gr, gx0), tags = _profiled(lambda: drv.backward(saved, True))
                assert tags == {"cfconv_bwd_pair_gs": L}, (label, name, bsplit, tags)
                (gr_e, _), tags_e = _profiled(lambda: drv.backward(saved, False))
                want = {"cfconv_bwd_pair_gs_geom": 1}
                if L > 1:
                    want["cfconv_bwd_pair_gs"] = L - 1
                assert tags_e == want, (label, name, bsplit, tags_e)
            gr, gx0, gr_e = gr.cpu(), gx0.cpu(), gr_e.cpu()
            for g_, what in ((gr, "gr"), (gr_e, "gr (eval call)")):
                assert torch.isfinite(g_).all(), (label, name, what, "entries never written", (~torch.isfinite(g_)).any(1).nonzero().flatten()[:8].tolist())
                assert (g_[beyond] == 0).all(), (label, name, what, "pairs at or beyond the cutoff")
            assert torch.isfinite(gx0).all()
            key = "%s bwd_%s" % (name, "split" if bsplit else "fp32")
            bad += _report(label + " " + key, "gradients", {"gr": B.max_norm_err(gr, ref["gr"]), "gr eval": B.max_norm_err(gr_e, ref["gr"]),
                                                            "gx0": B.max_norm_err(gx0, ref["gx0"])}, TOL)
            bad += _report(label + " " + key, "eval vs full", {"gr": B.max_norm_err(gr_e, gr)}, X_GRAD)
            out[bsplit] = (gr, gx0)
        res[name] = out
    for a, b in (("rowtile", "pair_split"), ("pair_split", "pair_fp32")):
        bad += _report(label, "%s vs %s" % (a, b), {"x_out": B.max_norm_err(res[a]["x"], res[b]["x"])}, X_OUT)
        bad += _report(label, "%s vs %s" % (a, b), {"gr": B.max_norm_err(res[a][True][0], res[b][True][0]),
                                                    "gx0": B.max_norm_err(res[a][True][1], res[b][True][1])}, X_GRAD)
    bad += _report(label, "bwd split vs fp32", {"gr": B.max_norm_err(res["pair_split"][True][0], res["pair_split"][False][0]),
                                                "gx0": B.max_norm_err(res["pair_split"][True][1], res["pair_split"][False][1])}, X_GRAD)
    assert not bad, bad
    return res


DRIVER_BASES = [(20, "gaussian", 3), (13, "bessel", 3), (20, "gaussian", 1), (8, "gaussian", 1), (13, "gaussian", 1), (16, "gaussian", 1), (32, "gaussian", 1),
                (20, "bessel", 1)]


@pytest.mark.parametrize("n_rbf,radial,n_layers", DRIVER_BASES)
@pytest.mark.parametrize("name", ["rows_last1", "rows_last32", "cutoff"])
def test_driver_saved_filters_on_the_row_edges(dev, name, n_rbf, radial, n_layers):
    """Forward with the filters saved (row-tile through edge_pair / half, pair kernels by tile), then the saved-filter backward with dL/dx0
    (cfconv_bwd_pair_gs) and without (cfconv_bwd_pair_gs_geom for the first interaction): filter rows, x_out, gr and gx0 against float64;
    the filter area outside the pairs keeps its sentinel; gr is assigned by the first backward kernel (it starts as NaN)."""
    c = {"rows_last1": lambda: B.rows(1), "rows_last32": lambda: B.rows(32), "cutoff": B.cutoff}[name]()
    _driver_case(c, n_rbf, radial, n_layers, dev, filtered=False)


@pytest.mark.parametrize("n_rbf,radial,n_layers", [(20, "gaussian", 3), (13, "bessel", 1), (32, "gaussian", 1)])
@pytest.mark.parametrize("live", [None, 0, 1, "none"])
def test_driver_on_compacted_lists(dev, live, n_rbf, radial, n_layers):
    """The pair filter on: the forward compacts the canonical pairs inside the cutoff (order kept) behind the filters; the count lands inside a
    tile, on a tile edge (32 k), one past it (32 k + 1) and at 0.  Filter rows are addressed by the position in the compacted list."""
    c = B.cutoff(live)
    n_live = len(B.live_pairs(c))
    assert {None: n_live % B.TILE > 1, 0: n_live % B.TILE == 0 and n_live > 0, 1: n_live % B.TILE == 1, "none": n_live == 0}[live]
    _driver_case(c, n_rbf, radial, n_layers, dev, filtered=True)


@pytest.mark.parametrize("n_rbf,radial", [(20, "gaussian"), (13, "bessel")])
def test_assigned_gr_equals_accumulated_gr(dev, n_rbf, radial):
    """Without the pair filter the first backward kernel ASSIGNS gr (no clearing pass); with it the driver clears gr and every kernel
    accumulates.  On a list with every pair inside the cutoff the compaction keeps every pair: the two must agree."""
    c = B.rows(1)
    got = {}
    for filtered in (False, True):
        drv = _Driver(c, n_rbf, radial, 3, dev, filtered)
        with _mode(-1, True):
            (x, saved), _ = _profiled(drv.forward)
            (gr, gx0), tags = _profiled(lambda: drv.backward(saved, True))
        assert tags == {"cfconv_bwd_pair_gs": 3}, tags
        if filtered:
            act, count = drv.compacted(saved.cpu())
            assert count == drv.n_half and np.array_equal(act.numpy(), B.canonical(c))
        got[filtered] = (x.cpu(), gr.cpu(), gx0.cpu())
        assert torch.isfinite(got[filtered][1]).all()
    bad = _report("rows_last1 n_rbf=%d %s" % (n_rbf, radial), "assigned vs accumulated", {"x_out": B.max_norm_err(got[False][0], got[True][0])}, X_OUT)
    bad += _report("rows_last1 n_rbf=%d %s" % (n_rbf, radial), "assigned vs accumulated",
                   {"gr": B.max_norm_err(got[False][1], got[True][1]), "gx0": B.max_norm_err(got[False][2], got[True][2])}, X_GRAD)
    assert not bad, bad


def test_driver_on_the_xcd_walks(dev):
    """The walk list through the driver, three interactions: the saved-filter kernels walk the tiles XCD-contiguously (4 097 tiles on 256
    compute units: a ragged last eighth), the row-tile forward saves through edge_pair while it walks the atoms.  Three interactions put filter
    areas at the offsets l x gsz, run cfconv_bwd_pair_gs both assigning and accumulating into gr, and the eval call ends with
    cfconv_bwd_pair_gs_geom on a gr that two interactions have already accumulated into (this covers what one interaction would)."""
    from schnetpack_amd import _lib
    c = B.walk(_lib.device_info()["compute_units"])
    assert c["info"]["pair_walk_live"] and c["info"]["row_walk_live"], c["info"]
    _driver_case(c, 20, "gaussian", 3, dev, filtered=False)
