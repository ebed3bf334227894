"""GPU: the branches of the cell-list neighbour search (csrc/spk_nbl.hip) that the common case never takes,
against the float64 brute-force oracle (oracle/nbl_oracle.py with ``extra_repeats="auto"``: nothing is wrapped
there) on the inputs of tests/nbl_edge_cases.py -- atoms whole cells outside the cell, pairs exactly at the
cutoff, rotated and left-handed cells, 63..200 atoms in one bin, 1..600 systems with empty ones, fewer bins
than the geometry allows, degenerate free geometry.  tests/test_nbl_edge_cases.py (CPU) shows that no input has
a distance within float32 round-off of its cutoff, so indices and integer shifts must be EQUAL to the oracle's.
"""
import pytest
import torch

import nbl_edge_cases as C
from oracle import nbl_oracle as NB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    return torch.device("cuda", 0)


def _hip_list(dev, case):
    """Device list of a case in canonical order; checks that idx_i ascends and rowptr is its CSR."""
    from schnetpack_amd import neighborlist as NL
    name, R, idx_m, cells, pbcs, cutoff = case
    out = NL.neighbor_list(R.to(dev), cutoff, idx_m.to(dev), cells.to(dev), pbcs.to(dev), n_systems=cells.shape[0], return_shifts=True)
    i, j = out["_idx_i"].cpu(), out["_idx_j"].cpu()
    Sh, off, rp = out["shifts"].cpu().long(), out["_offsets"].cpu(), out["rowptr"].cpu().long()
    assert bool((i[1:] >= i[:-1]).all()), name
    assert torch.equal(rp, torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(i, minlength=R.shape[0]).cumsum(0)])), name
    raw = (i, j, Sh, off)
    order = NB.canonical_order(i, j, Sh)
    return (i[order], j[order], Sh[order], off[order]), raw


@pytest.mark.parametrize("name", C.case_names())
def test_edge_case_equals_oracle(dev, name):
    case = C.case(name)
    _, R, idx_m, cells, pbcs, cutoff = case
    ref = C.reference(name)
    (i, j, Sh, off), raw = _hip_list(dev, case)
    assert i.shape == ref["idx_i"].shape, (name, i.shape[0], ref["idx_i"].shape[0])
    assert torch.equal(i, ref["idx_i"]) and torch.equal(j, ref["idx_j"]), name
    assert torch.equal(Sh, ref["S"]), name
    # offsets = S . cell: two fma and one product per component, each within half an ulp of a partial sum
    cm = cells.double()[idx_m[i]] if i.numel() else torch.zeros(0, 3, 3, dtype=torch.float64)
    bound = 4 * C.EPS32 * torch.einsum("ek,ekl->el", Sh.abs().double(), cm.abs())
    err = (off.double() - ref["offsets"]).abs()
    if i.numel() and float(bound.max()) > 0:
        print("%s: worst offset error / bound %.3f" % (name, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), (name, float((err - bound).max()))
    # symmetric: (j, i, -S) is there, with the negated offsets to the bit (+-0 compare equal)
    back = NB.canonical_order(j, i, -Sh)
    assert torch.equal(j[back], i) and torch.equal(i[back], j) and torch.equal(-Sh[back], Sh), name
    assert bool((off[back] == -off).all()), name
    # deterministic: a second build is bit-identical, order inside the rows included
    _, raw2 = _hip_list(dev, case)
    assert all(torch.equal(a, b) for a, b in zip(raw, raw2)), name
    assert bool((ref["d"] < cutoff).all())


@pytest.mark.parametrize("k", [k for k in range(30) if k not in C.WRAPPED_FAR])
def test_whole_cell_displacements_only_change_the_shifts(dev, k):
    """Device against device: the list of R0 + K.cell has the pairs of the in-cell R0, shifts S - K_j + K_i."""
    name, R0, K, cell, pbc, cutoff = C.wrapped_parts()[k]
    (i0, j0, S0, _), _ = _hip_list(dev, C.case("wrapped0[%d]" % k))
    (i1, j1, S1, _), _ = _hip_list(dev, C.case("wrapped[%d]" % k))
    want = S0 - K[j0] + K[i0]
    order = NB.canonical_order(i0, j0, want)
    assert torch.equal(i1, i0[order]) and torch.equal(j1, j0[order]) and torch.equal(S1, want[order])


def test_empty_systems_and_bad_molecule_indices(dev):
    from schnetpack_amd import neighborlist as NL
    from schnetpack_amd._lib import SpkHipError
    cells = (torch.eye(3) * 4.0).repeat(5, 1, 1).to(dev)
    pbcs = torch.ones(5, 3, dtype=torch.bool, device=dev)
    out = NL.neighbor_list(torch.zeros(0, 3, device=dev), 3.0, torch.zeros(0, dtype=torch.long, device=dev), cells, pbcs, n_systems=5)
    assert out["_idx_i"].numel() == 0 and out["rowptr"].cpu().tolist() == [0]
    # atoms in system 2 only: 0, 1, 3, 4 are empty
    R = torch.tensor([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5]], device=dev)
    out = NL.neighbor_list(R, 1.5, torch.tensor([2, 2], device=dev), cells, pbcs, n_systems=5, return_shifts=True)
    assert out["_idx_i"].cpu().tolist() == [0, 1] and out["_idx_j"].cpu().tolist() == [1, 0] and not bool(out["shifts"].any())
    R = torch.rand(4, 3, generator=torch.Generator().manual_seed(0)).to(dev)
    with pytest.raises(SpkHipError, match="outside"):         # idx_m beyond n_systems
        NL.neighbor_list(R, 2.0, torch.tensor([0, 0, 1, 5], device=dev), n_systems=2)
    with pytest.raises(SpkHipError, match="outside"):         # negative idx_m
        NL.neighbor_list(R, 2.0, torch.tensor([-1, 0, 0, 1], device=dev), n_systems=2)
    # the library is usable afterwards
    out = NL.neighbor_list(R, 2.0, torch.tensor([0, 0, 1, 1], device=dev), n_systems=2)
    assert out["_idx_i"].cpu().tolist() == [0, 1, 2, 3]


def test_transform_on_a_float64_sample_outside_the_cell(dev):
    """HipNeighborList on CPU float64 positions several cells outside a rotated cell: indices equal the oracle,
    offsets are S @ cell evaluated in float64."""
    from schnetpack_amd.neighborlist import HipNeighborList
    name, R, idx_m, cells, pbcs, cutoff = C.case("wrapped[4]")
    ref = C.reference(name)
    assert ref["idx_i"].shape[0] > 1000 and int(ref["S"].abs().max()) >= 3
    inp = {"_atomic_numbers": torch.ones(R.shape[0], dtype=torch.long), "_positions": R.double(),
           "_cell": cells.double().reshape(1, 3, 3), "_pbc": pbcs[0]}
    out = HipNeighborList(cutoff)(dict(inp))
    assert out["_idx_i"].device.type == "cpu" and out["_offsets"].dtype == torch.float64
    Sh = torch.round(out["_offsets"] @ torch.linalg.inv(cells[0].double())).long()
    order = NB.canonical_order(out["_idx_i"], out["_idx_j"], Sh)
    assert torch.equal(out["_idx_i"][order], ref["idx_i"]) and torch.equal(out["_idx_j"][order], ref["idx_j"]) and torch.equal(Sh[order], ref["S"])
    err = (out["_offsets"][order] - ref["offsets"]).abs().max() / ref["offsets"].abs().max()
    assert float(err) <= 1e-12


def _md_inputs(dev, case):
    _, R, idx_m, cells, pbcs, cutoff = case
    return {"_positions": R.to(dev), "_idx_m": idx_m.to(dev), "_n_atoms": torch.bincount(idx_m, minlength=cells.shape[0]).to(dev),
            "_cell": cells.to(dev), "_pbc": pbcs.reshape(-1).to(dev)}


def _as_set(i, j, off, cells, idx_m):
    S = torch.round(torch.einsum("el,elk->ek", off.double(), torch.linalg.inv(cells.double())[idx_m[i]])).long()
    order = NB.canonical_order(i, j, S)
    return i[order], j[order], S[order]


def test_md_list_of_a_batch_outside_its_cells(dev):
    """NeighborListMD on three systems with different rotated cells and atoms displaced out of them:
    (a) the filtered list is the oracle's at the bare cutoff, (b) one changed cell entry -> exactly one rebuild
    and the oracle's list for the new cell, (c) a changed atom count -> rebuild, (d) without the buffer filter
    the tensors handed out stay the same objects between rebuilds."""
    from schnetpack_amd.neighborlist import NeighborListMD
    case = C.case("md[3systems]")
    _, R, idx_m, cells, pbcs, cutoff = case
    inputs = _md_inputs(dev, case)
    md = NeighborListMD(C.MD_CUTOFF, C.MD_SHELL)

    def check(nb, name, cells, idx_m, n=None):
        ref = C.reference(name)
        ri, rj, rS = ref["idx_i"], ref["idx_j"], ref["S"]
        if n is not None:                       # the last atom left: its pairs leave with it, no other distance changes
            keep = (ri < n) & (rj < n)
            ri, rj, rS = ri[keep], rj[keep], rS[keep]
        got = _as_set(nb["_idx_i"].cpu(), nb["_idx_j"].cpu(), nb["_offsets"].cpu(), cells, idx_m)
        assert got[0].shape == ri.shape
        assert torch.equal(got[0], ri) and torch.equal(got[1], rj) and torch.equal(got[2], rS)

    check(md.get_neighbors(inputs), "md[3systems]", cells, idx_m)                      # (a)
    assert md.n_builds == 1 and C.reference("md[3systems]")["idx_i"].shape[0] > 200
    assert int(C.reference("md[3systems]")["S"].abs().max()) >= 3
    check(md.get_neighbors(inputs), "md[3systems]", cells, idx_m)
    assert md.n_builds == 1
    changed = C.case("md[3systems,cell_changed]")                                      # (b)
    inputs2 = _md_inputs(dev, changed)
    assert int((changed[3] != cells).sum()) == 1
    check(md.get_neighbors(inputs2), "md[3systems,cell_changed]", changed[3], idx_m)
    assert md.n_builds == 2
    check(md.get_neighbors(inputs2), "md[3systems,cell_changed]", changed[3], idx_m)
    assert md.n_builds == 2
    n = R.shape[0] - 1                                                                 # (c)
    inputs3 = dict(inputs2, _positions=inputs2["_positions"][:n], _idx_m=inputs2["_idx_m"][:n],
                   _n_atoms=torch.bincount(idx_m[:n], minlength=3).to(dev))
    check(md.get_neighbors(inputs3), "md[3systems,cell_changed]", changed[3], idx_m[:n], n=n)
    assert md.n_builds == 3
    keep = NeighborListMD(C.MD_CUTOFF, C.MD_SHELL, filter_buffer=False)                # (d)
    a = keep.get_neighbors(inputs)
    moved = dict(inputs, _positions=inputs["_positions"] + 0.01)
    b = keep.get_neighbors(moved)
    assert keep.n_builds == 1
    assert all(a[k].data_ptr() == b[k].data_ptr() and a[k].shape == b[k].shape for k in ("_idx_i", "_idx_j", "_offsets"))
    assert a["_idx_i"].shape[0] >= C.reference("md[3systems]")["idx_i"].shape[0]


@pytest.mark.parametrize("name", ["lattice[periodic,2.0]", "lattice[periodic_moved,2.0]", "lattice[periodic,2.0+ulp]", "lattice[periodic_moved,2.0+ulp]"])
def test_cutoff_is_strict(dev, name):
    """Simple-cubic lattice, spacing 1, every coordinate exact: 26 neighbours at cutoff 2.0 (the six at distance
    exactly 2.0 are outside), 32 at the next float32."""
    (i, j, Sh, off), _ = _hip_list(dev, C.case(name))
    assert torch.bincount(i, minlength=64).tolist() == [32 if name.endswith("+ulp]") else 26] * 64
