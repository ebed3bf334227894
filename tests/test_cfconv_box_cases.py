"""The lists of tests/cfconv_box_cases.py have the properties their docstrings state, and they are well-conditioned: the same formula
evaluated in float32 on the host stays at least 3x inside the bounds that tests/test_gpu_cfconv_box.py holds the device to (1e-5
against float64, by the max norm and per row) -- a device failure on these lists cannot be blamed on the inputs.  No GPU."""
import numpy as np
import pytest
import torch

import cfconv_box_cases as B

TOL, SPARE = 1e-5, 3.0
SYMMETRIC = [("rows", 1), ("rows", 32), ("cutoff", None), ("cutoff", 0), ("cutoff", 1), ("cutoff", "none")]


def _case(kind, arg):
    return B.rows(arg) if kind == "rows" else B.cutoff(arg)


@pytest.mark.parametrize("kind,arg", SYMMETRIC)
def test_symmetric_lists_are_sorted_and_antisymmetric(kind, arg):
    c = _case(kind, arg)
    ii, jj, r = c["idx_i"].numpy(), c["idx_j"].numpy(), c["r_ij"].numpy()
    assert c["N"] % B.ROW_WAVES != 0 and c["N"] <= 700
    key = ii * c["N"] + jj
    assert (np.diff(key) > 0).all() and (ii != jj).all()                  # idx_i ascending, idx_j ascending within a row, no duplicates
    rev = B.reverse_edges(c)
    assert (r[rev] == -r).all()                                             # both directions, opposite vectors bit for bit
    lengths = B.row_lengths(c)
    for want in B.ROW_LENGTHS:
        assert (lengths == want).any(), want
    iso = np.nonzero(lengths == 0)[0]
    assert iso[0] == 0 and iso[-1] == c["N"] - 1 and ((iso > 100) & (iso < c["N"] - 100)).any()   # start, middle and end of the atom range


@pytest.mark.parametrize("last_tile", [1, 32])
def test_rows_tile_and_run_patterns(last_tile):
    c = B.rows(last_tile)
    h = B.canonical(c)
    assert len(h) * 2 == len(c["idx_i"])
    assert (len(h) - 1) % B.TILE + 1 == last_tile
    s, e = B.half_runs(c)
    inside = (e % B.TILE != 0) & (s // B.TILE == (e - 1) // B.TILE)
    at_edge = e % B.TILE == 0
    spans = (e - 1) // B.TILE > s // B.TILE
    print("%s: %d atoms, %d pairs, %d runs: %d end inside a tile, %d at a tile edge, %d span tiles (longest %d)"
          % (c["info"]["name"], c["N"], len(h), len(s), inside.sum(), at_edge.sum(), spans.sum(), (e - s).max()))
    assert inside.any() and at_edge.any() and spans.any() and (e - s).max() > 2 * B.TILE
    assert ((s % B.TILE == 0) & (e - s == 64)).any()                       # the first star: a run that starts and ends on tile edges
    assert float(B.d32(c).max()) < B.CUTOFF


def test_cutoff_rows_and_special_pairs():
    c = B.cutoff()
    d, ii, jj = B.d32(c), c["idx_i"].numpy(), c["idx_j"].numpy()
    cut = np.float32(B.CUTOFF)
    assert d.min() > 0.89 and d.max() < 1.12 * B.CUTOFF + 1e-3
    ordinary = np.abs(d - cut) < 1e-4
    (i0, j0), (i1, j1) = c["info"]["exact_pair"], c["info"]["below_pair"]
    e_at = np.nonzero((ii == i0) & (jj == j0))[0][0]
    e_below = np.nonzero((ii == i1) & (jj == j1))[0][0]
    assert d[e_at] == cut and d[e_below] == np.nextafter(cut, np.float32(0)) and ordinary.sum() == 4    # the two pairs, both directions
    # with a fused multiply-add the norm of an axis-parallel vector is the same
    r = c["r_ij"].double().numpy()
    assert np.float32(np.sqrt(np.float32((r[e_below] ** 2).sum()))) == d[e_below]
    lengths = B.row_lengths(c)
    beyond = np.bincount(ii, weights=(d >= cut), minlength=c["N"])
    within = np.bincount(ii, weights=(d < cut), minlength=c["N"])
    long_rows = lengths >= 31
    assert (beyond[long_rows] >= 2).all() and (within[long_rows] >= 16).all()
    assert lengths[i0] == 97 and lengths[i1] == 97
    single = lengths == 1
    d_single = d[np.isin(ii, np.nonzero(single)[0])]
    assert ((d_single < B.D_SINGLE) | (d_single >= 1.01 * cut)).all() and (d_single >= cut).any() and (d_single < cut).any()


def test_compaction_variants_land_on_the_tile_edges():
    n = {live: len(B.live_pairs(B.cutoff(live))) for live in (None, 0, 1, "none")}
    print("canonical pairs inside the cutoff: %s of %d" % (n, len(B.canonical(B.cutoff()))))
    assert n[0] % B.TILE == 0 and n[0] > 0 and n[1] % B.TILE == 1 and n["none"] == 0
    assert n[None] % B.TILE not in (0, 1) and n[None] - B.TILE < n[0] <= n[None]
    for live in (0, 1, "none"):                                            # same structure as the drawn case
        assert torch.equal(B.cutoff(live)["idx_i"], B.cutoff()["idx_i"]) and torch.equal(B.cutoff(live)["idx_j"], B.cutoff()["idx_j"])
    assert float(B.d32(B.cutoff("none")).min()) >= B.CUTOFF


def test_asymmetric_rows_both_ways():
    c = B.asymmetric()
    ii, jj = c["idx_i"].numpy(), c["idx_j"].numpy()
    assert (np.diff(ii * c["N"] + jj) > 0).all() and c["N"] % B.ROW_WAVES != 0
    by_i, by_j = B.row_lengths(c), B.row_lengths(c, "idx_j")
    print("asymmetric: %d atoms, %d edges; rows 0 ... %d, by-neighbour rows 0 ... %d (%d above 32, %d empty)"
          % (c["N"], len(ii), by_i.max(), by_j.max(), (by_j > 32).sum(), (by_j == 0).sum()))
    for want in (0, 1, 31, 32, 33, 64, 65):
        assert (by_i == want).any()
    assert (by_j == 0).any() and (by_j > 64).any() and by_j[-1] == 0 and by_i[0] == 0
    d = B.d32(c)
    alone = (by_i[ii] == 1) | (by_j[jj] == 1)
    assert alone.any() and ((d[alone] < B.D_SINGLE) | (d[alone] >= B.CUTOFF)).all() and (d >= B.CUTOFF).any() and d.max() < 6.0
    key = set((ii * c["N"] + jj).tolist())
    assert any((j * c["N"] + i) not in key for i, j in zip(ii[:200], jj[:200]))      # not symmetric


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_walk_shape_conditions(cus):
    N, degree, cond = B.walk_shape(cus)
    print(cus, cond)
    assert N == 16385 and degree % 2 == 0
    assert cond["n_at_least_2_14"] and cond["n_not_multiple_of_8"] and cond["tiles_at_least_16_per_workgroup"] and cond["tiles_not_multiple_of_8"]
    if cus == 256:
        assert degree == 16 and cond["tiles"] == 4097 and cond["pair_walk_live"] and cond["row_walk_live"]
        c = B.walk(256)
        assert len(B.canonical(c)) == N * degree // 2 and (B.row_lengths(c) == degree).all()
        assert (c["r_ij"][B.reverse_edges(c)] == -c["r_ij"]).all()


# ---------------------------------------------------------------------------------------------------------
# conditioning: float32 on the host against float64
# ---------------------------------------------------------------------------------------------------------
def _conditioning(c, n_rbf, radial):
    p = B.filter_params(n_rbf)
    h, gy = B.features(c["N"], 11)
    ref = B.cfconv_ref(c, h, p, radial, gy=gy)
    got = B.cfconv_ref(c, h, p, radial, gy=gy, dtype=torch.float32)
    figs = {"y": B.max_norm_err(got["y"], ref["y"]), "gh": B.max_norm_err(got["gh"], ref["gh"]), "gr": B.max_norm_err(got["gr"], ref["gr"]),
            "y/row": B.per_row_err(got["y"], ref["y"], ref["scale_y"])[0], "gh/row": B.per_row_err(got["gh"], ref["gh"], ref["scale_gh"])[0]}
    print("%-14s n_rbf=%2d %-8s float32 host vs float64: %s  (bound %.1e / %g)"
          % (c["info"]["name"], n_rbf, radial, "  ".join("%s %.2e" % kv for kv in figs.items()), TOL, SPARE))
    return figs


@pytest.mark.parametrize("n_rbf,radial", B.BASES)
@pytest.mark.parametrize("name", ["rows", "cutoff", "asymmetric"])
def test_float32_host_formula_has_margin(name, n_rbf, radial):
    c = {"rows": B.rows, "cutoff": B.cutoff, "asymmetric": B.asymmetric}[name]()
    figs = _conditioning(c, n_rbf, radial)
    assert all(v < TOL / SPARE for v in figs.values()), figs


def test_float32_host_formula_has_margin_on_the_walk():
    figs = _conditioning(B.walk(256), 20, "gaussian")
    assert all(v < TOL / SPARE for v in figs.values()), figs


@pytest.mark.parametrize("n_rbf,radial,n_layers", [(20, "gaussian", 3), (13, "bessel", 3), (20, "gaussian", 1)])
def test_float32_host_representation_has_margin(n_rbf, radial, n_layers):
    rep = B.model_params(n_rbf, radial, n_layers)
    for c in (B.rows(), B.cutoff()):
        x0, gx = B.features(c["N"], 12)
        ref = B.representation_ref(c, x0, rep, n_layers, radial, gx_out=gx)
        got = B.representation_ref(c, x0, rep, n_layers, radial, gx_out=gx, dtype=torch.float32)
        figs = {k: B.max_norm_err(got[k], ref[k]) for k in ("x_out", "gr", "gx0")}
        print("%-14s n_rbf=%2d %-8s L=%d float32 host vs float64: %s" % (c["info"]["name"], n_rbf, radial, n_layers, "  ".join("%s %.2e" % kv for kv in figs.items())))
        assert all(v < TOL / SPARE for v in figs.values()), figs
        # filter rows of the pairs inside the cutoff, per pair against the row's max|ref|
        d = torch.from_numpy(B.d32(c)[B.live_pairs(c)])
        fp = B.filter_params(n_rbf)
        r64, r32 = B.filter_rows(d, fp, radial), B.filter_rows(d, fp, radial, torch.float32)
        worst = float(((r32.double() - r64).abs().amax(1) / r64.abs().amax(1)).max())
        print("   filter rows: worst pair %.2e" % worst)
        assert worst < TOL / SPARE


def test_block_evaluation_equals_one_block():
    c = B.rows()
    p = B.filter_params(20)
    h, gy = B.features(c["N"], 11)
    one, many = B.cfconv_ref(c, h, p, "gaussian", gy=gy, block=1 << 20), B.cfconv_ref(c, h, p, "gaussian", gy=gy, block=4099)
    for k in ("y", "gh", "gr"):
        assert B.max_norm_err(many[k], one[k]) < 1e-14
