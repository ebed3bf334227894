"""CPU restatement of the reference's neighbour-list semantics.  TEST INFRASTRUCTURE ONLY -- the
product path (schnetpack_amd.neighborlist -> libspk_hip.so) never imports this module.

Follows ``TorchNeighborList`` (transform/neighborlist.py:438-553, itself after TorchANI's aev.py):
brute force over all atom pairs and all cell shifts that can bring an image within the cutoff.
Pinned against the live reference class (tests/test_oracle_vs_reference.py) and against the
reference's own precomputed Argon vectors (tests/conftest.py:192-447 -> tests/golden/nbl_argon.npz).

The order of pairs inside a row is implementation defined in the reference (``torch.argsort`` of
idx_i, :448) and its own test compares after a canonical sort (tests/data/test_transforms.py:53-104);
``canonical_order`` is that sort with the integer shifts as the tie-breaker.
"""
from typing import Optional, Tuple

import torch

Tensor = torch.Tensor


def frac_floor_span(R: Tensor, cell: Tensor, pbc: Tensor) -> Tuple[int, int, int]:
    """``extra_repeats="auto"``: per periodic axis, max - min of floor(fractional coordinate) over the
    atoms (0 for atoms inside one cell, 0 along free axes) -- how many more repeats a pair of atoms that
    sit in different cell images can need on top of the in-cell count."""
    if R.shape[0] == 0:
        return (0, 0, 0)
    fl = torch.floor(R.double() @ torch.linalg.inv(cell.double()))
    span = (fl.max(0).values - fl.min(0).values).long()
    return tuple(int(v) if bool(p) else 0 for v, p in zip(span, pbc))


def half_space_shifts(cell: Tensor, pbc: Tensor, cutoff: float, extra_repeats=(0, 0, 0)) -> Tensor:
    """Integer shift vectors S != 0 of one half space (S and -S never both) that can hold images
    within ``cutoff`` (transform/neighborlist.py:509-553): n_k = ceil(cutoff * |k-th row of the
    reciprocal cell|) repeats along every periodic axis, plus ``extra_repeats[k]`` (the reference
    assumes atoms inside the cell; atoms that are whole cells apart need that many more)."""
    recip = torch.linalg.inv(cell).t()
    n = torch.ceil(cutoff * torch.linalg.norm(recip, dim=1)).long()
    n = n + torch.as_tensor([int(e) for e in extra_repeats], dtype=torch.long)
    n = torch.where(pbc.bool(), n, torch.zeros_like(n))
    rng = [torch.arange(-int(k), int(k) + 1) for k in n]
    S = torch.cartesian_prod(*rng)
    # lexicographically positive half: first non-zero component > 0
    first = torch.where(S[:, 0] != 0, S[:, 0], torch.where(S[:, 1] != 0, S[:, 1], S[:, 2]))
    return S[first > 0]


def neighbor_list(R: Tensor, cell: Optional[Tensor], pbc: Optional[Tensor], cutoff: float, extra_repeats=0
                  ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(idx_i, idx_j, S, offsets) of one system: every directed pair with
    ``|R_j - R_i + S.cell| < cutoff`` (strict, :492-493), ``offsets = S @ cell`` (:457), rows in
    canonical order.  ``extra_repeats``: 0 (the reference: atoms inside the cell), a per-axis int
    triple, or ``"auto"`` (:func:`frac_floor_span`) for atoms anywhere in space; S always refers to the
    positions as given.  Still brute force over pairs x shifts, nothing is wrapped."""
    n = R.shape[0]
    ar = torch.arange(n)
    periodic = pbc is not None and bool(torch.any(pbc))
    if periodic:
        if isinstance(extra_repeats, str):
            assert extra_repeats == "auto", extra_repeats
            extra_repeats = frac_floor_span(R, cell, pbc)
        elif isinstance(extra_repeats, int):
            extra_repeats = (extra_repeats,) * 3
        Sh = half_space_shifts(cell.to(R.dtype), pbc, cutoff, extra_repeats)
    else:
        Sh = torch.zeros(0, 3, dtype=torch.long)
        cell = torch.zeros(3, 3, dtype=R.dtype) if cell is None else cell
    cellf = cell.to(R.dtype)
    # central cell: unordered pairs i < j (:473-475); shifted cells: all ordered (i, j) (:480-484)
    pi0, pj0 = torch.combinations(ar).unbind(-1) if n > 1 else (ar[:0], ar[:0])
    vec = R[pi0] - R[pj0]                                            # :488-489
    keep = torch.linalg.norm(vec, dim=1) < cutoff                    # :492-493
    pi_l, pj_l, S_l = [pi0[keep]], [pj0[keep]], [torch.zeros(int(keep.sum()), 3, dtype=torch.long)]
    pi1, pj1 = torch.cartesian_prod(ar, ar).unbind(-1) if n else (ar[:0], ar[:0])
    d1 = R[pi1] - R[pj1]
    chunk = max(1, 2000000 // max(1, n * n))                         # shifts per pass: bounds the memory only
    for c0 in range(0, Sh.shape[0], chunk):
        Sc = Sh[c0:c0 + chunk]
        vec = d1[None, :, :] + (Sc.to(R.dtype) @ cellf)[:, None, :]
        s_idx, p_idx = torch.nonzero(torch.linalg.norm(vec, dim=2) < cutoff, as_tuple=True)
        pi_l.append(pi1[p_idx]); pj_l.append(pj1[p_idx]); S_l.append(Sc[s_idx])
    pi, pj, S_all = torch.cat(pi_l), torch.cat(pj_l), torch.cat(S_l)
    # both directions (:441-452): (i<-j, -S) and (j<-i, +S)
    idx_i = torch.cat([pi, pj])
    idx_j = torch.cat([pj, pi])
    S = torch.cat([-S_all, S_all])
    order = canonical_order(idx_i, idx_j, S)
    idx_i, idx_j, S = idx_i[order], idx_j[order], S[order]
    return idx_i, idx_j, S, S.to(R.dtype) @ cellf


def canonical_order(idx_i: Tensor, idx_j: Tensor, S: Tensor) -> Tensor:
    """Permutation sorting pairs by (i, j, Sx, Sy, Sz)."""
    if idx_i.numel() == 0:
        return torch.zeros(0, dtype=torch.long)
    smin = S.min()
    span = int(S.max() - smin) + 1
    n = int(max(idx_i.max(), idx_j.max())) + 1
    key = (((idx_i * n + idx_j) * span + (S[:, 0] - smin)) * span + (S[:, 1] - smin)) * span + (S[:, 2] - smin)
    return torch.argsort(key)


def batch_neighbor_list(R: Tensor, idx_m: Tensor, cells: Optional[Tensor], pbcs: Optional[Tensor], cutoff: float,
                        extra_repeats=0, n_sys: Optional[int] = None):
    """Per-system lists concatenated with the atom offset of each system added to the indices
    (what ``_atoms_collate_fn`` does, data/loader.py:35-46).  cells [M,3,3], pbcs [M,3]; ``n_sys``
    (default idx_m.max() + 1) lets the batch end in systems without atoms -- empty systems, wherever
    they are, contribute nothing."""
    if n_sys is None:
        n_sys = int(idx_m.max()) + 1 if idx_m.numel() else 0
    assert idx_m.numel() == 0 or int(idx_m.max()) < n_sys
    out_i, out_j, out_S, out_o = [], [], [], []
    for m in range(n_sys):
        sel = torch.nonzero(idx_m == m).flatten()
        if sel.numel() == 0:
            continue
        a0 = int(sel[0])
        i, j, S, o = neighbor_list(R[sel], None if cells is None else cells[m], None if pbcs is None else pbcs[m], cutoff, extra_repeats)
        out_i.append(i + a0); out_j.append(j + a0); out_S.append(S); out_o.append(o)
    if not out_i:
        z = torch.zeros(0, dtype=torch.long)
        return z, z, torch.zeros(0, 3, dtype=torch.long), torch.zeros(0, 3, dtype=R.dtype)
    return torch.cat(out_i), torch.cat(out_j), torch.cat(out_S), torch.cat(out_o)
