"""CPU: the inputs of tests/test_gpu_nbl_edges.py are what they claim to be, and the extended oracle is sound.

* every case stays out of the float32 guard band around its cutoff (tests/nbl_edge_cases.py), so "device list
  == float64 oracle" is a fair demand;
* every builder reaches the branch it was written for, judged by a NumPy restatement of the bin geometry of
  csrc/spk_nbl.hip (bins per axis, "never more bins than atoms", reach, wraps, atoms per bin);
* ``extra_repeats`` changes nothing for in-cell atoms, the oracle equals the live TorchNeighborList there, and
  displacing atoms by whole cell vectors changes the oracle's shifts by exactly ``-K_j + K_i``.
"""
import numpy as np
import pytest
import torch

import nbl_edge_cases as C
from oracle import nbl_oracle as NB
from oracle import refshim

ALL = C.case_names()
IN_CELL = [c[0] for c in C.wrapped_in_cell()]


@pytest.mark.parametrize("name", ALL + IN_CELL)
def test_guard_band(name):
    band, d = C.guard_band(name)
    cutoff = C.case(name)[5]
    gap = (d - cutoff).abs()
    # exempt: distances that are exact in float32 and float64 alike (C.EXACT_AT_CUTOFF) -- the integer 2.0 of the
    # lattice against the cutoffs 2.0 and nextafter(2.0), the integer 6.0 of the images of a single atom
    exact = (d == round(cutoff)) if name in C.EXACT_AT_CUTOFF else torch.zeros_like(gap, dtype=torch.bool)
    assert not bool(((gap < band) & ~exact).any()), (name, band, float(gap[~exact].min()))
    # the band covers the float32 evaluation of the distance: 3 subtractions, 3 additions of S.cell (two fma and a
    # product each), 3 squares, 2 sums and a square root stay below 16 half-ulps of the largest magnitude involved
    assert band >= 16 * C.EPS32 * cutoff


def test_case_inventory():
    assert len(ALL) == len(set(ALL))
    assert [n for n in ALL if n.startswith("wrapped")] == ["wrapped[%d]" % k for k in range(30)]
    assert len([n for n in ALL if n.startswith("lattice")]) == 12
    assert len([n for n in ALL if n.startswith("dense[blob")]) == 7 and len([n for n in ALL if n.startswith("dense[cube")]) == 6
    for name, R, idx_m, cells, pbcs, cutoff in C.all_cases():
        assert R.dtype == torch.float32 and idx_m.dtype == torch.int64 and cells.dtype == torch.float32 and pbcs.dtype == torch.bool
        assert R.shape == (idx_m.shape[0], 3) and cells.shape[1:] == (3, 3) and pbcs.shape == (cells.shape[0], 3)
        assert bool((idx_m[1:] >= idx_m[:-1]).all()) and (idx_m.numel() == 0 or int(idx_m.max()) < cells.shape[0])


def test_wrapped_reaches_the_integer_wrap_path():
    parts = C.wrapped_parts()
    dets, patterns, n_outside = [], set(), 0
    for k, (name, R0, K, cell, pbc, rc) in enumerate(parts):
        g = C.geometry(name)[0]
        assert bool((cell != 0).all()), name                                # rotated: all nine entries
        dets.append(g["det"])
        patterns.add(tuple(pbc.tolist()))
        assert bool(pbc.any())
        assert np.array_equal(g["wrap"] != 0, (g["wrap"] != 0) & g["pbc"][None, :])
        n_outside += int((g["wrap"] != 0).any(1).sum())
        lim = 50 if k in C.WRAPPED_FAR else 3
        assert int(K.abs().max()) <= lim
        # in-cell R0 (up to float32 rounding at the faces): the kernel's wrap is K, or K -+ 1 for an atom on a face
        assert int(np.abs(g["wrap"] - K.numpy()).max()) <= 1, name
        assert 1 <= R0.shape[0] <= 60
    assert sum(d < 0 for d in dets) == 15 and sum(d > 0 for d in dets) == 15
    assert len(patterns) >= 6
    assert n_outside > 500
    assert all(int(np.abs(C.geometry("wrapped[%d]" % k)[0]["wrap"]).max()) >= 30 for k in C.WRAPPED_FAR)
    assert max(p[1].shape[0] for p in parts) >= 50 and min(p[1].shape[0] for p in parts) == 1


def test_lattice_is_exact_and_sits_on_the_cutoff():
    for name in [n for n in ALL if n.startswith("lattice")]:
        _, R, idx_m, cells, pbcs, cutoff = C.case(name)
        assert torch.equal(R, R.round()) and torch.equal(cells[0], torch.eye(3) * 4.0)
        ref = C.reference(name)
        d2 = (ref["d"] ** 2)
        assert float((d2 - d2.round()).abs().max()) < 1e-12                 # integer squared distances
        at = int((ref["d"] == 2.0).sum())
        assert (at == 0) if cutoff == 2.0 else (at > 0 and cutoff == C.CUT2_NEXT)
        g = C.geometry(name)[0]
        if "periodic" in name:
            per_atom = torch.bincount(ref["idx_i"], minlength=64)
            assert per_atom.tolist() == [26 if cutoff == 2.0 else 32] * 64
            if cutoff == 2.0:
                assert g["nb"] == [2, 2, 2] and g["reach"] == [2, 2, 2] and all(float(h) == cutoff for h in g["hb"])
            else:
                assert g["nb"] == [1, 1, 1]
        if "moved" in name and "free" not in name:
            w = g["wrap"][:, g["pbc"]]
            assert set(np.unique(w[:, 0])) == {-2} and set(np.unique(w[:, 1])) == {3}
    assert C.CUT2_NEXT > 2.0 and np.float32(C.CUT2_NEXT) == np.nextafter(np.float32(2.0), np.float32(3.0))


def test_dense_puts_every_atom_in_one_bin():
    for n in C.DENSE_COUNTS:
        g = C.geometry("dense[blob,%d]" % n)[0]
        assert g["nb"] == [1, 1, 1] and g["occupancy"] == n and g["natoms"] == n
    assert C.geometry("dense[blob,200]")[0]["occupancy"] > 128
    for n in C.DENSE_COUNTS[:-1]:
        g = C.geometry("dense[cube,%d]" % n)[0]
        assert g["nb"] == [1, 1, 1] and g["occupancy"] == n and g["reach"] == [2, 2, 2]
        ref = C.reference("dense[cube,%d]" % n)
        assert int((ref["idx_i"] == ref["idx_j"]).sum()) > 0                # self images
        assert ref["idx_i"].shape[0] < 150000


def test_batches_have_empty_systems_and_cross_the_scan_width():
    sizes = {}
    for name in [n for n in ALL if n.startswith("batches")]:
        _, R, idx_m, cells, pbcs, cutoff = C.case(name)
        n_sys = cells.shape[0]
        counts = torch.bincount(idx_m, minlength=n_sys)
        sizes[name] = n_sys
        assert int(counts.max()) <= 4
        if n_sys >= 40:
            empty = (counts == 0)
            assert bool(empty[0]) and bool(empty[-2:].all()) and bool(empty[7:10].all()) and not bool(empty[1])
            assert n_sys < 255 or 0.08 < float(empty.float().mean()) < 0.25         # about 15 % (binomial scatter at 255 draws)
            per = pbcs.all(1)
            assert bool(per.any()) and bool((~pbcs.any(1)).any())
            assert 3.0 <= float(cells[:, [0, 1, 2], [0, 1, 2]].min()) and float(cells.max()) <= 6.0
    assert sorted(sizes.values()) == [1, 45, 255, 256, 257, 260, 600]
    # past the scan width of k_nbl_binoffsets: a system >= 256 with atoms whose block-local bin offset is that of a
    # non-empty system of the first block (257 -> bin offset 1 = system 1; both hold four atoms near their origins)
    _, R, idx_m, cells, pbcs, cutoff = C.case("batches[260]")
    counts = torch.bincount(idx_m, minlength=260)
    assert int(counts[257]) == 4 and int(counts[1]) == 4 and C.geometry("batches[260]")[0]["nb"] == [1, 1, 1] and C.geometry("batches[260]")[256]["nb"] == [1, 1, 1]
    cross = torch.cdist(R[idx_m == 1].double(), R[idx_m == 257].double())
    assert float(cross.min()) < cutoff - 0.5
    counts = torch.bincount(C.case("batches[600]")[2], minlength=600)
    assert int((counts[256:] > 0).sum()) > 200
    _, R, idx_m, cells, pbcs, cutoff = C.case("batches[40+5unused]")
    assert cells.shape[0] > int(idx_m.max()) + 1
    assert C.reference("batches[600]")["idx_i"].shape[0] > 1000


def test_sparse_clips_the_bins_to_the_atom_count():
    want = {"sparse[cube100]": [1, 1, 1], "sparse[rod200x6x6]": [35, 1, 1], "sparse[slab20x20,z60]": [2, 2, 7], "sparse[chain80]": [12, 1, 1]}
    for name, nb in want.items():
        g = C.geometry(name)[0]
        assert int(np.prod(g["nb_geom"])) > g["natoms"] >= int(np.prod(g["nb"])), name
        assert g["nb"] == nb, (name, g["nb"])
        assert C.reference(name)["idx_i"].shape[0] > 0
    # the chain needs the trim loop after the common rescale: floor(26 * cbrt(12 / 26)) = 20 > 12
    assert int(np.floor(np.float32(26) * np.cbrt(np.float32(12) / np.float32(26)))) > 12
    assert C.case("sparse[cube100]")[1].shape[0] == 7 and C.reference("sparse[cube100]")["idx_i"].shape[0] == 6
    assert bool((C.reference("sparse[cube100]")["S"] != 0).any(0).all())   # one pair through every periodic face


def test_degenerate_geometry():
    assert C.geometry("degenerate[collinear]")[0]["fext"].tolist()[1:] == [0.0, 0.0]
    g = C.geometry("degenerate[collinear]")[0]
    assert float(g["hb"][0]) == C.case("degenerate[collinear]")[5]         # free axis with hb == cutoff
    assert C.geometry("degenerate[coplanar]")[0]["fext"].tolist()[2] == 0.0
    assert C.geometry("degenerate[coincident]")[0]["fext"].tolist() == [0.0, 0.0, 0.0]
    assert C.reference("degenerate[coincident]")["idx_i"].shape[0] == 20 and float(C.reference("degenerate[coincident]")["d"].max()) == 0.0
    for name in ("degenerate[one_atom_cube1.5]", "degenerate[one_atom_height1.2]"):
        g = C.geometry(name)[0]
        assert g["natoms"] == 1 and max(g["reach"]) >= 4
        ref = C.reference(name)
        assert ref["idx_i"].shape[0] > 50 and bool((ref["S"] != 0).any(1).all())
    assert min(float(h) for h in C.geometry("degenerate[one_atom_height1.2]")[0]["hb"]) == pytest.approx(1.2, abs=1e-5)
    ref = C.reference("degenerate[pair_through_shift]")
    assert ref["idx_i"].tolist() == [0, 1] and ref["S"].tolist() == [[-1, 0, 0], [1, 0, 0]]
    assert C.geometry("degenerate[frac_rounds_to_one]")[0]["fixups"] == 1
    assert float(C.case("degenerate[far_molecule]")[1].abs().min(0).values.max()) >= 1000.0


@pytest.mark.parametrize("name", IN_CELL)
def test_extra_repeats_change_nothing_for_atoms_inside_the_cell(name):
    _, R, idx_m, cells, pbcs, cutoff = C.case(name)
    base = NB.neighbor_list(R.double(), cells[0].double(), pbcs[0], cutoff)
    for extra in ("auto", (2, 1, 3), 1):
        got = NB.neighbor_list(R.double(), cells[0].double(), pbcs[0], cutoff, extra_repeats=extra)
        assert all(torch.equal(a, b) for a, b in zip(got, base)), (name, extra)
    ref = C.reference(name)
    assert torch.equal(ref["idx_i"], base[0]) and torch.equal(ref["idx_j"], base[1]) and torch.equal(ref["S"], base[2])


def test_batch_oracle_with_empty_systems():
    _, R, idx_m, cells, pbcs, cutoff = C.case("batches[40+5unused]")
    a = NB.batch_neighbor_list(R.double(), idx_m, cells.double(), pbcs, cutoff, n_sys=cells.shape[0])
    b = NB.batch_neighbor_list(R.double(), idx_m, cells.double()[:int(idx_m.max()) + 1], pbcs[:int(idx_m.max()) + 1], cutoff)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    z = NB.batch_neighbor_list(torch.zeros(0, 3, dtype=torch.float64), torch.zeros(0, dtype=torch.long), cells.double(), pbcs, cutoff, n_sys=cells.shape[0])
    assert z[0].numel() == 0 and z[2].shape == (0, 3)


@pytest.mark.parametrize("k", range(30))
def test_oracle_shifts_follow_whole_cell_displacements(k):
    """List of R0 + K.cell (float64, not rounded) == list of R0 with S' = S - K_j + K_i."""
    name, R0, K, cell, pbc, cutoff = C.wrapped_parts()[k]
    i0, j0, S0, _ = NB.neighbor_list(R0.double(), cell.double(), pbc, cutoff)
    R = R0.double() + K.double() @ cell.double()
    i1, j1, S1, o1 = NB.neighbor_list(R, cell.double(), pbc, cutoff, extra_repeats="auto")
    want = S0 - K[j0] + K[i0]
    order = NB.canonical_order(i0, j0, want)
    assert torch.equal(i1, i0[order]) and torch.equal(j1, j0[order]) and torch.equal(S1, want[order])
    d = torch.linalg.norm(R[j1] - R[i1] + o1, dim=1)
    assert i1.numel() == 0 or float(d.max()) < cutoff
    if k not in C.WRAPPED_FAR:
        # the float32 inputs of the device check (wrapped[k] against wrapped0[k]) fall into the same class
        a, b = C.reference("wrapped[%d]" % k), C.reference("wrapped0[%d]" % k)
        wantb = b["S"] - K[b["idx_j"]] + K[b["idx_i"]]
        ob = NB.canonical_order(b["idx_i"], b["idx_j"], wantb)
        assert torch.equal(a["idx_i"], b["idx_i"][ob]) and torch.equal(a["idx_j"], b["idx_j"][ob]) and torch.equal(a["S"], wantb[ob])


ONE_PAIR = ["wrapped0[23]"]


def test_oracle_equals_live_torch_neighbor_list_on_general_cells():
    """TorchNeighborList itself (transform/neighborlist.py:438-553) on the rotated / left-handed cells with the
    atoms folded back into the cell."""
    if not refshim.available():
        pytest.skip("reference sources not present")
    ns = refshim.load()
    if ns.neighborlist is None:
        pytest.skip("reference neighbour-list module not importable: %s" % ns.neighborlist_error)
    # the reference squeezes its hit index (:502) and fails on exactly one undirected pair: those systems, by name
    one_pair = [name for name in IN_CELL if C.reference(name)["idx_i"].shape[0] == 2]
    assert one_pair == ONE_PAIR
    for name in IN_CELL:
        if name in ONE_PAIR:
            continue
        _, R, idx_m, cells, pbcs, cutoff = C.case(name)
        R, cell, pbc = R.double(), cells[0].double(), pbcs[0]
        out = ns.neighborlist.TorchNeighborList(cutoff)({"_atomic_numbers": torch.ones(R.shape[0], dtype=torch.long), "_positions": R,
                                                         "_cell": cell.reshape(1, 3, 3), "_pbc": pbc})
        i, j, off = out["_idx_i"], out["_idx_j"], out["_offsets"]
        S = torch.round(off @ torch.linalg.inv(cell)).long()
        order = NB.canonical_order(i, j, S)
        ref = C.reference(name)
        assert torch.equal(i[order], ref["idx_i"]) and torch.equal(j[order], ref["idx_j"]) and torch.equal(S[order], ref["S"]), name
        assert torch.allclose(off[order], ref["offsets"], atol=1e-9), name
