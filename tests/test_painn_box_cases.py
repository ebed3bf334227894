"""The lists of tests/painn_box_cases.py have the properties their docstrings state, and they are well-conditioned: the PaiNN message
formula evaluated in float32 on the host stays at least 2x inside every bound that tests/test_gpu_painn_box.py holds the device to
(1e-5 against float64, by the max norm and per row) on every case and basis -- a device failure on these lists cannot be blamed on the
inputs.  No GPU; nothing here depends on an EdgePlan.

Why 2x and not the 3x of the cfconv lists.  Two terms are the same in ANY float32 arithmetic and sit between 3.3e-6 and 5e-6 here.  The
phase k pi d / r_c of the highest of 20 Bessel functions reaches 50 rad at d = 4 A; half an ulp of that is 1.9e-6 rad, and a row whose
only pair lies there (d < D_SINGLE) shows it undamped, since PaiNN's filter is one linear layer: up to 4.3e-6 of the row on the
inherited lists (about 100 such rows each).  `hubs`, with 900 such rows, draws its live spokes below 2.5 A for this reason
(painn_box_cases.py).  And dL/dr through a Gaussian basis of 24 functions (width 0.22 A) carries the rounding of d itself, (d - mu_k) /
w^2 x 3e-7: up to 4.3e-6 of max|gr| on `hubs`, where every pair stands alone.  The figures are printed."""
import numpy as np
import pytest
import torch

import painn_box_cases as B

TOL, SPARE = 1e-5, 2.0
LISTS = {"rows_last1": lambda: B.rows(1), "rows_last32": lambda: B.rows(32), "cutoff": B.cutoff, "cutoff_0": lambda: B.cutoff(0),
         "cutoff_1": lambda: B.cutoff(1), "cutoff_none": lambda: B.cutoff("none"), "asymmetric": B.asymmetric}
LISTS.update({"hubs_%s" % ("drawn" if v is None else v): (lambda v=v: B.hubs(v)) for v in B.HUB_LIVE})


# ---------------------------------------------------------------------------------------------------------
# structure
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("live", B.HUB_LIVE)
def test_hubs_rows_sit_on_both_sides_of_the_live_cap(live):
    c = B.hubs(live)
    ii, jj, r = c["idx_i"].numpy(), c["idx_j"].numpy(), c["r_ij"].numpy()
    N = c["N"]
    assert N == 921 and N % B.ROW_WAVES != 0 and N % 8 != 0
    assert (np.diff(ii * N + jj) > 0).all() and (ii != jj).all()                 # rows ascending, neighbours ascending within a row
    assert (r[B.reverse_edges(c)] == -r).all()                                    # antisymmetric bit for bit
    lengths = B.row_lengths(c)
    c256, c257, c300, c34, c66 = c["info"]["centres"]
    assert (lengths[c256], lengths[c257], lengths[c300], lengths[c34], lengths[c66]) == (B.RT_LIVE_CAP, B.RT_LIVE_CAP + 1, 300, 34, 66)
    assert set(lengths.tolist()) == {0, 1, 34, 66, 256, 257, 300}
    assert lengths[0] == 0 and lengths[-1] == 0 and lengths[-2] == 0
    d = B.d32(c)
    assert ((d < B.HUB_D_NEAR) | (d >= np.float32(1.01 * B.CUTOFF) - 1e-4)).all() and B.HUB_D_NEAR <= B.D_SINGLE and d.min() > 0.89 and d.max() < 1.12 * B.CUTOFF + 1e-3
    assert torch.equal(c["idx_i"], B.hubs()["idx_i"]) and torch.equal(c["idx_j"], B.hubs()["idx_j"])
    n_live = B.live_row_counts(c)
    print("%s: live pairs of the centre rows %d / %d / %d" % (c["info"]["name"], n_live[c256], n_live[c257], n_live[c300]))
    if live == "all":
        assert (n_live == lengths).all() and n_live[c256] == B.RT_LIVE_CAP
        return
    if live is None:
        assert 32 < n_live[c256] < 256 and n_live[c256] % 32 not in (0, 1)
    else:
        assert n_live[c256] == live
    for cen in (c257, c300):                                                      # pairs on both sides of the cutoff in the uncompacted rows
        assert 64 < n_live[cen] < lengths[cen] - 32
        rows_d = d[ii == cen]
        for s in range(0, len(rows_d), 32):                                       # ... in every chunk of 32 but possibly the last
            chunk = rows_d[s:s + 32]
            if len(chunk) == 32:
                assert (chunk < B.CUTOFF).any() and (chunk >= B.CUTOFF).any(), (cen, s)
    assert torch.equal(c["idx_i"], B.hubs()["idx_i"]) and torch.equal(c["idx_j"], B.hubs()["idx_j"])


def test_inherited_lists_keep_their_row_lengths_and_cutoff_pairs():
    """What the PaiNN suite relies on in the lists it takes from the cfconv module (asserted in full by tests/test_cfconv_box_cases.py)."""
    for c in (B.rows(1), B.rows(32), B.cutoff(), B.cutoff(0), B.cutoff(1), B.cutoff("none")):
        lengths = B.row_lengths(c)
        for want in (0, 1, 31, 32, 33, 63, 64, 65, 96, 97):                # (34 and 66 are rows of `hubs`)
            assert (lengths == want).any(), (c["info"]["name"], want)
        assert c["N"] % B.ROW_WAVES != 0
    c = B.cutoff()
    d, ii, jj = B.d32(c), c["idx_i"].numpy(), c["idx_j"].numpy()
    cut = np.float32(B.CUTOFF)
    (i0, j0), (i1, j1) = c["info"]["exact_pair"], c["info"]["below_pair"]
    assert d[np.nonzero((ii == i0) & (jj == j0))[0][0]] == cut and d[np.nonzero((ii == j0) & (jj == i0))[0][0]] == cut
    assert d[np.nonzero((ii == i1) & (jj == j1))[0][0]] == np.nextafter(cut, np.float32(0))
    assert (B.live_row_counts(B.cutoff("none")) == 0).all()
    a = B.asymmetric()
    by_i, by_j = B.row_lengths(a), B.row_lengths(a, "idx_j")
    for want in (0, 1, 31, 32, 33, 64, 65):
        assert (by_i == want).any()
    assert (by_j == 0).any() and (by_j > 64).any()


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_walk_shape_conditions(cus):
    N, degree, cond = B.walk_shape(cus)
    print(cus, cond)
    assert N >= 1 << 14 and N % 8 != 0 and degree in (2, 4)
    assert cond["n_at_least_2_14"] and cond["n_not_multiple_of_8"] and cond["eighth_not_multiple_of_step"] and cond["tiles_not_multiple_of_8"]
    assert cond["row_walk_live"] and cond["tile_walk_live"]
    if cus == 256:
        assert (N, degree, cond["tiles"], cond["row_grid"], cond["atom_step"], cond["atoms_per_xcd"]) == (16385, 2, 1025, 512, 256, 2049)
        c = B.walk(256)
        assert len(c["idx_i"]) == N * degree and (B.row_lengths(c) == degree).all()
        assert (c["r_ij"][B.reverse_edges(c)] == -c["r_ij"]).all() and float(B.d32(c).max()) < B.D_SINGLE


# ---------------------------------------------------------------------------------------------------------
# the measures
# ---------------------------------------------------------------------------------------------------------
def test_per_row_measure_sees_what_the_max_norm_hides():
    """A padding pair counted into the one-pair row next to the 300-pair row: invisible in the tensor's max norm, 100 % of the row."""
    c = B.hubs()
    x = B.inputs(c["N"])
    wf, bf = B.filter_params(20)
    ref = B.message_ref(c, x["c"], x["q"], x["mu"], wf, bf, 20, "gaussian")
    leaf = c["info"]["centres"][2] + 1
    while ref["scale_q"][leaf] == 0:
        leaf += 1
    got = ref["q_out"].clone()
    got[leaf] += ref["dq"][leaf]                     # the row's only pair counted twice
    assert B.max_norm_err(got, ref["q_out"]) < 0.05
    fig, row, dead = B.per_row_err(got, x["q"], ref["dq"], ref["scale_q"])
    assert row == leaf and fig > 0.5 and not dead
    dead_row = int((ref["scale_q"] == 0).nonzero()[0])
    got = ref["q_out"].clone()
    got[dead_row, 3] += 1e-12
    assert B.per_row_err(got, x["q"], ref["dq"], ref["scale_q"])[2] == [dead_row]
    assert B.per_row_err(ref["q_out"], x["q"], ref["dq"], ref["scale_q"])[0] < 1e-15


def test_block_evaluation_equals_one_block():
    c = B.cutoff()
    x = B.inputs(c["N"])
    wf, bf = B.filter_params(20)
    one = B.message_ref(c, x["c"], x["q"], x["mu"], wf, bf, 20, "gaussian", gq=x["gq"], gmu=x["gmu"], block=1 << 20)
    many = B.message_ref(c, x["c"], x["q"], x["mu"], wf, bf, 20, "gaussian", gq=x["gq"], gmu=x["gmu"], block=4099)
    for k in ("q_out", "mu_out", "gc", "gmu_in", "gr", "scale_q", "scale_mu", "scale_gc", "scale_gmu"):
        assert B.max_norm_err(many[k], one[k]) < 1e-13, k


def test_message_formula_is_the_oracle_interaction():
    """message_ref against oracle.spk_oracle.painn_interaction's sums (the same reference lines, written independently)."""
    from oracle import spk_oracle as O
    c = B.asymmetric()
    x = {k: v.double() for k, v in B.inputs(c["N"]).items()}
    wf, bf = B.filter_params(20)
    r = c["r_ij"].double()
    d = torch.sqrt((r * r).sum(1, keepdim=True))
    off, w = O.gaussian_rbf_params(20, B.CUTOFF)
    Wij = O.dense(O.gaussian_rbf(d, off.double(), w.double()), wf.double(), bf.double()) * O.cosine_cutoff(d, B.CUTOFF)[..., None]
    m = Wij * x["c"].unsqueeze(1)[c["idx_j"]]
    dq = O.scatter_add(m[..., :B.NF], c["idx_i"], c["N"]).squeeze(1)
    dmu = O.scatter_add(m[..., B.NF:2 * B.NF] * (r / d)[..., None] + m[..., 2 * B.NF:] * x["mu"][c["idx_j"]], c["idx_i"], c["N"])
    ref = B.message_ref(c, x["c"], x["q"], x["mu"], wf, bf, 20, "gaussian")
    assert B.max_norm_err(ref["q_out"], x["q"] + dq) < 1e-14 and B.max_norm_err(ref["mu_out"], x["mu"] + dmu) < 1e-14


# ---------------------------------------------------------------------------------------------------------
# conditioning: float32 on the host against float64
# ---------------------------------------------------------------------------------------------------------
def _conditioning(c, n_rbf, radial, mu_zero=False):
    x = B.inputs(c["N"])
    wf, bf = B.filter_params(n_rbf)
    mu = None if mu_zero else x["mu"]
    ref = B.message_ref(c, x["c"], x["q"], mu, wf, bf, n_rbf, radial, gq=x["gq"], gmu=x["gmu"])
    got = B.message_ref(c, x["c"], x["q"], mu, wf, bf, n_rbf, radial, gq=x["gq"], gmu=x["gmu"], dtype=torch.float32)
    figs = {k: B.max_norm_err(got[k], ref[k]) for k in ("q_out", "mu_out", "gc", "gmu_in", "gr")}
    dead = []
    for k, base, s, scale in (("q_out", x["q"], "dq", "scale_q"), ("mu_out", mu, "dmu", "scale_mu"), ("gc", None, "gc", "scale_gc"),
                              ("gmu_in", x["gmu"], "dgmu", "scale_gmu")):
        fig, _, bad = B.per_row_err(got[k], base, ref[s], ref[scale])
        figs[k + "/row"] = fig
        dead += bad
    beyond = torch.from_numpy(B.d32(c) >= np.float32(B.CUTOFF))
    assert not dead and (got["gr"][beyond] == 0).all() and (ref["gr"][beyond] == 0).all()
    print("%-14s n_rbf=%2d %-8s%s float32 host vs float64: %s  (bound %.1e / %g)"
          % (c["info"]["name"], n_rbf, radial, " mu0" if mu_zero else "", "  ".join("%s %.2e" % kv for kv in figs.items()), TOL, SPARE))
    return figs


@pytest.mark.parametrize("n_rbf,radial", B.BASES + B.DECLINED)
@pytest.mark.parametrize("name", sorted(LISTS))
def test_float32_host_formula_has_margin(name, n_rbf, radial):
    figs = _conditioning(LISTS[name](), n_rbf, radial)
    assert all(v < TOL / SPARE for v in figs.values()), figs


def test_float32_host_formula_has_margin_on_the_walk():
    figs = _conditioning(B.walk(256), 20, "gaussian")
    assert all(v < TOL / SPARE for v in figs.values()), figs


@pytest.mark.parametrize("n_rbf,radial", [(20, "gaussian"), (24, "gaussian"), (20, "bessel")])
@pytest.mark.parametrize("n_layers", [1, 2])
@pytest.mark.parametrize("name", ["rows_last1", "cutoff", "hubs_drawn", "asymmetric"])
def test_float32_host_representation_has_margin(name, n_layers, n_rbf, radial):
    c = LISTS[name]()
    P = B.model_params(n_rbf, radial, n_layers)
    x = B.inputs(c["N"], seed=22)
    ref = B.representation_ref(c, x["q"], P, n_layers, n_rbf, radial, gq_out=x["gq"], gmu_out=x["gmu"])
    got = B.representation_ref(c, x["q"], P, n_layers, n_rbf, radial, gq_out=x["gq"], gmu_out=x["gmu"], dtype=torch.float32)
    geo = B.representation_ref(c, x["q"], P, n_layers, n_rbf, radial, gq_out=x["gq"], gmu_out=x["gmu"], want_gq0=False)
    assert "gq0" not in geo and torch.equal(geo["gr"], ref["gr"])                # gr does not depend on whether gq0 is asked for
    figs = {k: B.max_norm_err(got[k], ref[k]) for k in ("q", "mu", "gr", "gq0")}
    f64, f32 = ref["first"], got["first"]
    figs["q1/row"] = B.per_row_err(f32["q_out"], x["q"], f64["dq"], f64["scale_q"])[0]
    figs["mu1/row"] = B.per_row_err(f32["mu_out"], None, f64["dmu"], f64["scale_mu"])[0]
    print("%-12s n_rbf=%2d %-8s L=%d float32 host vs float64: %s" % (c["info"]["name"], n_rbf, radial, n_layers, "  ".join("%s %.2e" % kv for kv in figs.items())))
    assert all(v < TOL / SPARE for v in figs.values()), figs
