"""The box-regime PaiNN message kernels (csrc/spk_painn_tile.hip, dispatch in csrc/spk_painn.hip) on the row and tile edges of
tests/painn_box_cases.py: the row-tile forward and backward, the 32-pair MFMA tile kernels in split and fp32 form, the row kernel with
and without its LDS radial table, the two-pass (TS + GEOM) backward of asymmetric lists in row and row-tile form, the MU0 and
geometry-only instances the representation driver chooses, the compaction of skin lists on both sides of RT_LIVE_CAP and both
XCD-contiguous walks -- none of them through the molecule-resident or block kernels (plans without groups or block plans; asserted by
profile tag).

Bounds.  Against the float64 formula the project's 1e-5, measured twice on every summed output: max|got - ref| / max|ref| over the
tensor, and per row max_c |(got - input term) - sum_ref| / (the row's own sum of absolute contributions, maximised over channels).  gr by
the max norm.  Rows without a pair inside the cutoff equal their input term exactly, dL/dr of pairs at or beyond the cutoff is exactly
0, and the row-tile, row and TS / GEOM paths are bit-equal over two launches.  Between two device paths the figures are printed, not
asserted.  Every figure is printed before it is asserted; the worst per case and kernel are recorded in profiles/painn_box_edges.md.

The driver level goes through the ctypes structs of schnetpack_amd/_lib.py (spk_painn_forward_f32 / spk_painn_backward_f32 with a
PainnT built here): the operator library derives its own plan, with groups, from the index tensors."""
import ctypes

import numpy as np
import pytest
import torch

import painn_box_cases as B

pytestmark = pytest.mark.gpu
TOL = 1e-5
NAN = float("nan")

# family -> (rowtile, tile, row_table, split, simple)
FAMILIES = {"rowtile": (1, -1, 0, True, False), "tile_split": (-1, 1, 0, True, False), "tile_fp32": (-1, 1, 0, False, False),
            "row": (-1, -1, 0, True, False), "row_lt": (-1, -1, 1, True, False), "simple": (-1, -1, 0, True, True)}
BIT_EQUAL = ("rowtile", "row", "row_lt")          # no atomics: a fixed summation order


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _family:
    """The switches of one kernel family for the calls inside; all restored on exit."""

    def __init__(self, name):
        self.rowtile, self.tile, self.table, self.split, self.simple = FAMILIES[name]

    def __enter__(self):
        from schnetpack_amd import _lib
        L = _lib.lib()
        self.before = (_lib.get_split(), _lib.get_variant())
        _lib.set_split(self.split)
        _lib.set_variant(_lib.VARIANT_SIMPLE if self.simple else _lib.VARIANT_AUTO)
        L.spk_painn_set_rowtile(self.rowtile); L.spk_painn_set_tile(self.tile); L.spk_painn_set_row_table(self.table)

    def __exit__(self, *exc):
        from schnetpack_amd import _lib
        L = _lib.lib()
        L.spk_painn_set_rowtile(0); L.spk_painn_set_tile(0); L.spk_painn_set_row_table(-1)
        _lib.set_split(bool(self.before[0])); _lib.set_variant(self.before[1])


def _profiled(fn):
    """Run fn() with the launch profile on: (result, {tag: count}) of the PaiNN message kernels; no molecule-resident or block kernel."""
    from schnetpack_amd import _lib
    _lib.profile_enable(True)
    _lib.profile_report()
    try:
        res = fn()
        torch.cuda.synchronize()
        rep = _lib.profile_report()
    finally:
        _lib.profile_enable(False)
    assert not any(("painn_mol" in t) or ("_blk" in t) for t in rep), rep
    return res, {t: c[0] for t, c in rep.items() if t.startswith("painn_msg_")}


def _radial(n_rbf, radial, dev):
    from schnetpack_amd import _lib, ops
    ps = [p.float().contiguous().to(dev) for p in B.radial_params(n_rbf, radial)]
    kind = _lib.SPK_RBF_GAUSSIAN if radial == "gaussian" else _lib.SPK_RBF_BESSEL
    return ops.radial_struct(kind, n_rbf, ps[0], ps[1] if len(ps) > 1 else None, B.CUTOFF), ps


def _plan(c, dev, filtered=False, transposed=False):
    from schnetpack_amd import ops
    plan = ops.EdgePlan(c["idx_i"].to(dev), c["idx_j"].to(dev), c["N"], c["r_ij"].to(dev), want_groups=False)
    assert plan.sorted and plan.groups is None and plan.blocks is None
    if transposed:
        plan.build_transposed()
    if filtered:
        plan.set_filter(True)
    return plan


def _report(label, what, figs, bound=None):
    print("%-52s %-26s %s%s" % (label, what, "  ".join("%s %.3e" % kv for kv in figs.items()), "  (bound %.1e)" % bound if bound else "  (recorded)"))
    return [(label, what, k, v) for k, v in figs.items() if bound is not None and not v < bound]


def _check_rows(label, what, got, base, ref_sum, ref_full, scale):
    got = got.cpu()
    assert torch.isfinite(got).all(), (label, what, "unwritten or non-finite rows", (~torch.isfinite(got.reshape(got.shape[0], -1))).any(1).nonzero().flatten()[:8].tolist())
    fig, row, dead = B.per_row_err(got, base, ref_sum, scale)
    assert not dead, (label, what, "rows without a pair inside the cutoff differ from their input term", dead[:8])
    return _report(label, "%s (worst row %d)" % (what, row), {"max-norm": B.max_norm_err(got.reshape(ref_full.shape), ref_full), "per-row": fig}, TOL)


def _expected(family, n_rbf, F, E, symmetric, transposed):
    """The tags a family's request ends in (a declined request falls to the row kernel; csrc/spk_painn.hip msg_dispatch)."""
    kpb = n_rbf // 8 + 1
    rt = F == 128 and kpb in (3, 4)
    if family == "simple":
        return {"painn_msg_fwd_simple"}, {"painn_msg_bwd_simple"}
    if family == "rowtile":
        fwd = {"painn_msg_fwd_rowtile"} if rt else {"painn_msg_fwd_row"}
    elif family in ("tile_split", "tile_fp32"):
        fwd = {"painn_msg_fwd_tile"} if (3 <= kpb <= 5 and E >= 32) else {"painn_msg_fwd_row"}
    else:
        fwd = {"painn_msg_fwd_row"}
    if not symmetric:
        if not transposed:
            return fwd, {"painn_msg_bwd_simple"}
        return fwd, ({"painn_msg_bwd_rowtile_t", "painn_msg_bwd_rowtile_geom"} if (family == "rowtile" and rt) else {"painn_msg_bwd_row_tsum", "painn_msg_bwd_row_geom"})
    if family == "rowtile" and rt:
        return fwd, {"painn_msg_bwd_rowtile_g", "painn_msg_bwd_rowtile_t"}
    if family in ("tile_split", "tile_fp32") and kpb in (3, 4) and E >= 32:
        return fwd, {"painn_msg_bwd_tile"}
    return fwd, {"painn_msg_bwd_row"}


# ---------------------------------------------------------------------------------------------------------
# a. operator level
# ---------------------------------------------------------------------------------------------------------
class _Op:
    """spk_painn_message_fwd_f32 / _bwd_f32 on a case, outputs into NaN-filled buffers (gr is accumulated into: it starts at 0)."""

    def __init__(self, c, n_rbf, radial, dev, F=B.NF, filtered=False, transposed=False):
        self.c, self.dev, self.F, self.N, self.E = c, dev, F, c["N"], len(c["idx_i"])
        self.plan = _plan(c, dev, filtered=filtered, transposed=transposed)
        self.rb, self.keep = _radial(n_rbf, radial, dev)
        self.x = B.inputs(self.N, F)
        self.wf, self.bf = B.filter_params(n_rbf, F)
        self.d = {k: v.contiguous().to(dev) for k, v in self.x.items()}
        self.wfd, self.bfd, self.rd = self.wf.contiguous().to(dev), self.bf.contiguous().to(dev), c["r_ij"].contiguous().to(dev)

    def fwd(self):
        from schnetpack_amd import _lib
        f, d = _lib.fptr, self.d
        q_out = torch.full((self.N, self.F), NAN, device=self.dev)
        mu_out = torch.full((self.N, 3, self.F), NAN, device=self.dev)
        _lib.check(_lib.lib().spk_painn_message_fwd_f32(self.plan.graph(), ctypes.byref(self.rb), f(d["c"]), f(d["q"]), f(d["mu"]), f(self.rd), f(self.wfd), f(self.bfd),
                                                        self.F, f(q_out), f(mu_out), _lib.stream()))
        return q_out, mu_out

    def bwd(self):
        from schnetpack_amd import _lib
        f, d = _lib.fptr, self.d
        gc = torch.full((self.N, 3 * self.F), NAN, device=self.dev)
        gmu_in = torch.full((self.N, 3, self.F), NAN, device=self.dev)
        gr = torch.zeros(self.E, 3, device=self.dev)
        _lib.check(_lib.lib().spk_painn_message_bwd_f32(self.plan.graph(), ctypes.byref(self.rb), f(d["c"]), f(d["mu"]), f(d["gq"]), f(d["gmu"]), f(self.rd), f(self.wfd),
                                                        f(self.bfd), self.F, f(gc), f(gmu_in), f(gr), _lib.stream()))
        return gc, gmu_in, gr


def _reference(c, n_rbf, radial, F=B.NF):
    x = B.inputs(c["N"], F)
    wf, bf = B.filter_params(n_rbf, F)
    return B.message_ref(c, x["c"], x["q"], x["mu"], wf, bf, n_rbf, radial, gq=x["gq"], gmu=x["gmu"])


def _operator_case(c, n_rbf, radial, dev, ref, families, F=B.NF, filtered=False, transposed=False, symmetric=True, backward_only=False):
    label = "%s%s%s F=%d n_rbf=%d %s" % (c["info"]["name"], " filtered" if filtered else "", " +transposed" if transposed else "", F, n_rbf, radial)
    op = _Op(c, n_rbf, radial, dev, F=F, filtered=filtered, transposed=transposed)
    assert op.plan.symmetric == symmetric
    x = op.x
    beyond = torch.from_numpy(B.d32(c) >= np.float32(B.CUTOFF))
    bad, outs = [], {}
    for fam in families:
        want_f, want_b = _expected(fam, n_rbf, F, op.E, symmetric, transposed)
        with _family(fam):
            res = {}
            if not backward_only:
                (q_out, mu_out), tags = _profiled(op.fwd)
                assert set(tags) == want_f, (label, fam, tags, want_f)
                if fam in BIT_EQUAL:
                    again = op.fwd()
                    assert torch.equal(q_out, again[0]) and torch.equal(mu_out, again[1]), (label, fam, "the forward is not bit-reproducible")
                bad += _check_rows(label + " " + fam, "q_out", q_out, x["q"], ref["dq"], ref["q_out"], ref["scale_q"])
                bad += _check_rows(label + " " + fam, "mu_out", mu_out, x["mu"], ref["dmu"], ref["mu_out"], ref["scale_mu"])
                res.update(q_out=q_out.cpu(), mu_out=mu_out.cpu())
            (gc, gmu_in, gr), tags = _profiled(op.bwd)
            assert set(tags) == want_b, (label, fam, tags, want_b)
            if fam in BIT_EQUAL and want_b != {"painn_msg_bwd_simple"}:
                again = op.bwd()
                assert all(torch.equal(a_, b_) for a_, b_ in zip((gc, gmu_in, gr), again)), (label, fam, "the backward is not bit-reproducible")
            bad += _check_rows(label + " " + fam, "gc", gc, None, ref["gc"], ref["gc"], ref["scale_gc"])
            bad += _check_rows(label + " " + fam, "gmu_in", gmu_in, x["gmu"], ref["dgmu"], ref["gmu_in"], ref["scale_gmu"])
            gr = gr.cpu()
            assert torch.isfinite(gr).all(), (label, fam, "gr")
            assert (gr[beyond] == 0).all(), (label, fam, "dL/dr of pairs at or beyond the cutoff", (gr[beyond] != 0).any(1).nonzero().flatten()[:8].tolist())
            bad += _report(label + " " + fam, "gr", {"max-norm": B.max_norm_err(gr, ref["gr"])}, TOL)
            res.update(gc=gc.cpu(), gmu_in=gmu_in.cpu(), gr=gr)
            outs[fam] = res
    base = "row" if "row" in outs else families[0]
    for fam in families:                       # between device paths: recorded, not asserted
        if fam != base:
            _report(label, "%s vs %s" % (fam, base), {k: B.max_norm_err(outs[fam][k], outs[base][k]) for k in outs[fam]})
    assert not bad, bad
    return outs


SYMMETRIC = {"rows_last1": lambda: B.rows(1), "rows_last32": lambda: B.rows(32), "cutoff": B.cutoff, "cutoff_0": lambda: B.cutoff(0),
             "cutoff_1": lambda: B.cutoff(1), "cutoff_none": lambda: B.cutoff("none")}
ALL_FAMILIES = tuple(FAMILIES)


@pytest.mark.parametrize("n_rbf,radial", B.BASES + B.DECLINED)
@pytest.mark.parametrize("name", sorted(SYMMETRIC))
def test_operator_on_the_row_edges(dev, name, n_rbf, radial):
    """Rows of 0, 1, 31 ... 33, 63 ... 65, 96, 97 pairs; with `cutoff` pairs on both sides of the cutoff in every long row, one pair exactly at it and
    one an ulp below, and (cutoff_none) rows whose pairs all lie beyond it: every kernel family, forward and backward, against float64 per
    tensor and per row.  n_rbf 15 and 32 are declined requests: the tag that ran is asserted (32 keeps the forward tile kernel)."""
    c = SYMMETRIC[name]()
    _operator_case(c, n_rbf, radial, dev, _reference(c, n_rbf, radial), ALL_FAMILIES)


@pytest.mark.parametrize("n_rbf,radial", B.BASES + B.DECLINED)
@pytest.mark.parametrize("live", B.HUB_LIVE)
def test_operator_on_the_hubs(dev, live, n_rbf, radial):
    """Rows of 256, 257 and 300 pairs (and 34, 66) with pairs on both sides of the cutoff, plain and as a skin plan: with the pair filter on the
    256-row is compacted (to 190 live pairs as drawn, to exactly 0, 1, 32, 33, or -- "all" -- to a list full to its last entry) and the 257- and
    300-rows take the uncompacted branch."""
    c = B.hubs(live)
    n_live = B.live_row_counts(c)[c["info"]["centres"][0]]
    assert n_live == {None: 190, "all": B.RT_LIVE_CAP}.get(live, live)
    ref = _reference(c, n_rbf, radial)
    plain = _operator_case(c, n_rbf, radial, dev, ref, ALL_FAMILIES)
    skin = _operator_case(c, n_rbf, radial, dev, ref, ("rowtile", "tile_split", "row", "row_lt"), filtered=True)
    for fam in skin:
        _report(c["info"]["name"], "%s: skin vs plain" % fam, {k: B.max_norm_err(skin[fam][k], plain[fam][k]) for k in skin[fam]})


@pytest.mark.parametrize("n_rbf,radial", B.BASES + B.DECLINED)
def test_operator_on_an_asymmetric_list(dev, n_rbf, radial):
    """Sorted asymmetric list: before its by-neighbour copy is attached the backward is the edge-parallel kernel with atomics; after it the TS pass
    over the by-neighbour rows (0 ... 150 pairs) and the GEOM pass over the rows, in row-tile form with the switch on and in row form with it
    off.  The forward needs no symmetry: every family runs it."""
    c = B.asymmetric()
    ref = _reference(c, n_rbf, radial)
    _operator_case(c, n_rbf, radial, dev, ref, ("rowtile", "row"), symmetric=False, backward_only=True)
    _operator_case(c, n_rbf, radial, dev, ref, ("rowtile", "tile_split", "tile_fp32", "row", "row_lt", "simple"), transposed=True, symmetric=False)


@pytest.mark.parametrize("name", ["rows_last1", "cutoff"])
def test_operator_with_64_features(dev, name):
    """F = 64: the tile and row kernels have the instance, the row-tile kernels decline (asserted by tag)."""
    c = SYMMETRIC[name]()
    _operator_case(c, 20, "gaussian", dev, _reference(c, 20, "gaussian", F=64), ("rowtile", "tile_split", "tile_fp32", "row", "simple"), F=64)


# ---------------------------------------------------------------------------------------------------------
# c. walks
# ---------------------------------------------------------------------------------------------------------
def test_operator_on_the_xcd_walks(dev):
    """A ring list sized for the device so that the row-tile and row kernels walk the atoms and the tile kernels walk the tiles XCD-contiguously,
    with N % 8 != 0, a last eighth that is no multiple of the per-XCD step and a tile count that is no multiple of 8."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N, degree, cond = B.walk_shape(cus)
    print(cus, cond)
    if not (cond["row_walk_live"] and cond["tile_walk_live"]):
        pytest.skip("no ring list makes both XCD walks ragged on %d compute units: %s" % (cus, cond))
    c = B.walk(cus)
    assert c["info"]["n_at_least_2_14"] and c["info"]["n_not_multiple_of_8"] and c["info"]["eighth_not_multiple_of_step"] and c["info"]["tiles_not_multiple_of_8"]
    assert c["info"]["row_walk_live"] and c["info"]["tile_walk_live"]
    _operator_case(c, 20, "gaussian", dev, _reference(c, 20, "gaussian"), ("rowtile", "tile_split", "tile_fp32", "row", "row_lt"))


# ---------------------------------------------------------------------------------------------------------
# b. driver level: the MU0 and geometry-only instances
# ---------------------------------------------------------------------------------------------------------
class _Driver:
    """spk_painn_forward_f32 / spk_painn_backward_f32 started from given scalar features, through a PainnT built from B.model_params (one filter
    slice per interaction, packed weights as the operator library attaches them).  Scratch after the forward of ONE interaction still
    holds that interaction's message outputs: q1 at [N F, 2 N F), mu1 at [2 N F, 5 N F)."""

    def __init__(self, c, n_rbf, radial, n_layers, dev, filtered=False, transposed=False):
        from schnetpack_amd import _lib
        self._lib, self.lib, self.c, self.dev, self.L = _lib, _lib.lib(), c, dev, n_layers
        self.N, self.E, F = c["N"], len(c["idx_i"]), B.NF
        self.P = B.model_params(n_rbf, radial, n_layers)
        self.plan = _plan(c, dev, filtered=filtered, transposed=transposed)
        D = lambda t: t.float().contiguous().to(dev)
        self.keep = []
        layers = (_lib.PainnLayerT * n_layers)()
        for l in range(n_layers):
            a, m = "interactions.%d.interatomic_context_net." % l, "mixing.%d." % l
            t = {"ctx_w1": self.P[a + "0.weight"], "ctx_b1": self.P[a + "0.bias"], "ctx_w2": self.P[a + "1.weight"], "ctx_b2": self.P[a + "1.bias"],
                 "filt_w": self.P["filter_net.weight"][3 * F * l:3 * F * (l + 1)], "filt_b": self.P["filter_net.bias"][3 * F * l:3 * F * (l + 1)],
                 "mix_w": self.P[m + "mu_channel_mix.weight"], "ictx_w1": self.P[m + "intraatomic_context_net.0.weight"],
                 "ictx_b1": self.P[m + "intraatomic_context_net.0.bias"], "ictx_w2": self.P[m + "intraatomic_context_net.1.weight"],
                 "ictx_b2": self.P[m + "intraatomic_context_net.1.bias"]}
            t.update({k + "T": t[k].t() for k in ("ctx_w1", "ctx_w2", "mix_w", "ictx_w1", "ictx_w2")})
            for name, w in t.items():
                wd = D(w)
                self.keep.append(wd)
                setattr(layers[l], name, wd.data_ptr())
        self.layers = layers
        self.m = _lib.PainnT(F, n_layers, 1e-8, 0, layers, None)
        n_pack = int(self.lib.spk_painn_packed_floats(ctypes.byref(self.m)))
        assert n_pack > 0
        self.wpack = torch.empty(n_pack, dtype=torch.float32, device=dev)
        _lib.check(self.lib.spk_painn_pack_weights_f32(ctypes.byref(self.m), _lib.fptr(self.wpack), _lib.stream()))
        self.m.wpack = self.wpack.data_ptr()
        self.rb, self.rkeep = _radial(n_rbf, radial, dev)
        self.n_saved = int(self.lib.spk_painn_saved_floats(ctypes.byref(self.m), self.N))
        self.n_scratch = int(self.lib.spk_painn_scratch_floats(ctypes.byref(self.m), self.N))
        self.x = B.inputs(self.N, seed=22)
        self.q0d, self.gqd, self.gmud = (self.x[k].contiguous().to(dev) for k in ("q", "gq", "gmu"))
        self.rd = c["r_ij"].contiguous().to(dev)

    def forward(self):
        _lib, f = self._lib, self._lib.fptr
        q = torch.full((self.N, B.NF), NAN, device=self.dev)
        mu = torch.full((self.N, 3, B.NF), NAN, device=self.dev)
        self.saved = torch.full((self.n_saved,), NAN, device=self.dev)
        self.scratch = torch.full((self.n_scratch,), NAN, device=self.dev)
        _lib.check(self.lib.spk_painn_forward_f32(ctypes.byref(self.m), self.plan.graph(), ctypes.byref(self.rb), f(self.q0d), f(self.rd), f(q), f(mu), f(self.saved),
                                                  f(self.scratch), _lib.stream()))
        return q, mu

    def backward(self, want_gq0):
        _lib, f = self._lib, self._lib.fptr
        gr = torch.full((self.E, 3), NAN, device=self.dev)           # the driver clears it itself
        gq0 = torch.full((self.N, B.NF), NAN, device=self.dev) if want_gq0 else None
        _lib.check(self.lib.spk_painn_backward_f32(ctypes.byref(self.m), self.plan.graph(), ctypes.byref(self.rb), f(self.gqd), f(self.gmud), f(self.rd), f(self.saved),
                                                   f(self.scratch), f(gr), f(gq0), _lib.stream()))
        return gr, gq0


def _counts(**kw):
    return {"painn_msg_" + k: v for k, v in kw.items() if v > 0}


def _driver_expected(fam, L, symmetric):
    """(forward, full backward, backward without dL/dq0) tag counts of an L-interaction call: the first interaction runs the MU0 instances (own
    tag in the forward), the last backward launch of the eval call is geometry-only."""
    if fam == "rowtile":
        fwd = _counts(fwd_rowtile_mu0=1, fwd_rowtile=L - 1)
        if symmetric:
            return fwd, _counts(bwd_rowtile_g=L, bwd_rowtile_t=L), _counts(bwd_rowtile_geom=1, bwd_rowtile_g=L - 1, bwd_rowtile_t=L - 1)
        return fwd, _counts(bwd_rowtile_geom=L, bwd_rowtile_t=L), _counts(bwd_rowtile_geom=L, bwd_rowtile_t=L - 1)
    fwd = _counts(fwd_tile_mu0=1, fwd_tile=L - 1) if fam == "tile_split" else _counts(fwd_row_mu0=1, fwd_row=L - 1)
    if not symmetric:                        # the two-pass backward has no tile form
        return fwd, _counts(bwd_row_geom=L, bwd_row_tsum=L), _counts(bwd_row_geom=L, bwd_row_tsum=L - 1)
    if fam == "tile_split":
        return fwd, _counts(bwd_tile=L), _counts(bwd_tile_geom=1, bwd_tile=L - 1)
    return fwd, _counts(bwd_row=L), _counts(bwd_row_geom=1, bwd_row=L - 1)


DRIVER_LISTS = {"rows_last1": (lambda: B.rows(1), False, True), "cutoff": (B.cutoff, False, True), "hubs_filtered": (B.hubs, True, True),
                "asymmetric_transposed": (B.asymmetric, False, False)}


@pytest.mark.parametrize("n_rbf,radial", [(20, "gaussian"), (24, "gaussian"), (20, "bessel")])
@pytest.mark.parametrize("n_layers", [1, 2])
@pytest.mark.parametrize("name", sorted(DRIVER_LISTS))
def test_driver_first_interaction_and_geometry_only(dev, name, n_layers, n_rbf, radial):
    """The representation driver from given features, 1 and 2 interactions with their own filter slices: the first interaction runs the MU0
    instance of the forward (and of the TS pass on the asymmetric list), the eval call (no dL/dq0) ends in the geometry-only launch alone for
    that interaction -- in row-tile, tile and row form, by tag.  q, mu, gr and gq0 against the float64 representation; with one interaction
    also the message outputs per row (from the driver's scratch); gr of the geometry-only call against gr of the full call."""
    make, filtered, symmetric = DRIVER_LISTS[name]
    c = make()
    label = "%s n_rbf=%d %s L=%d" % (name, n_rbf, radial, n_layers)
    drv = _Driver(c, n_rbf, radial, n_layers, dev, filtered=filtered, transposed=not symmetric)
    assert drv.plan.symmetric == symmetric
    x = drv.x
    ref = B.representation_ref(c, x["q"], drv.P, n_layers, n_rbf, radial, gq_out=x["gq"], gmu_out=x["gmu"])
    first = ref["first"]
    beyond = torch.from_numpy(B.d32(c) >= np.float32(B.CUTOFF))
    nf = drv.N * B.NF
    bad, res = [], {}
    for fam in ("rowtile", "tile_split", "row"):
        want_f, want_b, want_e = _driver_expected(fam, n_layers, symmetric)
        with _family(fam):
            (q, mu), tags = _profiled(drv.forward)
            assert tags == want_f, (label, fam, tags, want_f)
            q, mu = q.cpu(), mu.cpu()
            assert torch.isfinite(q).all() and torch.isfinite(mu).all(), (label, fam, "q / mu")
            bad += _report(label + " " + fam, "representation", {"q": B.max_norm_err(q, ref["q"]), "mu": B.max_norm_err(mu, ref["mu"])}, TOL)
            if n_layers == 1:
                sc = drv.scratch.cpu()
                bad += _check_rows(label + " " + fam, "message q1", sc[nf:2 * nf].view(drv.N, B.NF), x["q"], first["dq"], first["q_out"], first["scale_q"])
                bad += _check_rows(label + " " + fam, "message mu1", sc[2 * nf:5 * nf].view(drv.N, 3, B.NF), None, first["dmu"], first["mu_out"], first["scale_mu"])
            (gr, gq0), tags = _profiled(lambda: drv.backward(True))
            assert tags == want_b, (label, fam, tags, want_b)
            (gr_e, _), tags_e = _profiled(lambda: drv.backward(False))
            assert tags_e == want_e, (label, fam, tags_e, want_e)
        gr, gq0, gr_e = gr.cpu(), gq0.cpu(), gr_e.cpu()
        for g_, what in ((gr, "gr"), (gr_e, "gr (geometry-only call)")):
            assert torch.isfinite(g_).all(), (label, fam, what, (~torch.isfinite(g_)).any(1).nonzero().flatten()[:8].tolist())
            assert (g_[beyond] == 0).all(), (label, fam, what, "pairs at or beyond the cutoff")
        assert torch.isfinite(gq0).all()
        bad += _report(label + " " + fam, "gradients", {"gr": B.max_norm_err(gr, ref["gr"]), "gr geom": B.max_norm_err(gr_e, ref["gr"]), "gq0": B.max_norm_err(gq0, ref["gq0"])}, TOL)
        bad += _report(label + " " + fam, "geometry-only vs full", {"gr": B.max_norm_err(gr_e, gr)}, TOL)
        res[fam] = {"q": q, "mu": mu, "gr": gr, "gq0": gq0}
    for fam in ("rowtile", "tile_split"):
        _report(label, "%s vs row" % fam, {k: B.max_norm_err(res[fam][k], res["row"][k]) for k in res[fam]})
    assert not bad, bad
