"""Seeded inputs that reach the rarely taken branches of the cell-list neighbour search (csrc/spk_nbl.hip):
atoms outside the cell, pairs exactly at the cutoff, rotated / left-handed cells, more than 64 and 128 atoms in
a bin, more than 256 systems with empty ones, fewer bins than the geometry allows, degenerate free geometry.
Shared by tests/test_nbl_edge_cases.py (CPU: the builders reach what they claim and stay out of the guard
band) and tests/test_gpu_nbl_edges.py (device list == oracle).  A plain module: no fixtures, no pytest hooks.

A case is ``(name, R float32 [N,3], idx_m int64 [N], cells float32 [M,3,3], pbcs bool [M,3], cutoff)``; the
number of systems is ``cells.shape[0]`` (systems without atoms are legal).

Guard band.  The kernel evaluates ``|R_j - R_i + S.cell|`` in float32, the oracle in float64 on the same float32
inputs.  ``band = 16 * 2**-24 * (max|R| + max|S.cell| + cutoff)`` bounds the float32 evaluation error with room
to spare; no case has an oracle distance with ``0 < |d - cutoff| < band`` (a condition on the INPUTS, asserted
on the CPU; a seed that violates it is replaced by another seed, see the *_SEEDS tables), and ``d == cutoff``
occurs only in the lattice cases where coordinates, differences and the square root are exact in both
precisions.
"""
import functools
import math

import numpy as np
import torch

from oracle import nbl_oracle as NB

EPS32 = 2.0 ** -24


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _rotation(g):
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))[None, :]
    if torch.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _one(name, R, cell, pbc, cutoff):
    R = R.float()
    return (name, R, torch.zeros(R.shape[0], dtype=torch.long), cell.float().reshape(1, 3, 3),
            torch.as_tensor(pbc, dtype=torch.bool).reshape(1, 3), float(cutoff))


# ---------------------------------------------------------------------------------------------------------
# wrapped: general cells, atoms displaced by whole cell vectors
# ---------------------------------------------------------------------------------------------------------
# one seed per system (1000 + k); the three whose system had a distance inside the guard band use seed + 100
WRAPPED_SEEDS = [1000 + k + (100 if k in (5, 21, 22) else 0) for k in range(30)]
WRAPPED_FAR = {27: (40, [True, False, False]), 28: (10, [True, True, False]), 29: (3, [True, True, True])}   # +-50 cells


@functools.lru_cache(maxsize=None)
def wrapped_parts():
    """[(name, R0 float32 in-cell along the periodic axes, K int64 [n,3], cell float32, pbc, cutoff)]."""
    out = []
    for k, seed in enumerate(WRAPPED_SEEDS):
        g = _gen(seed)
        n = int(torch.randint(1, 61, (1,), generator=g))
        lengths = 2.5 + 7.5 * torch.rand(3, generator=g, dtype=torch.float64)
        tri = torch.diag(lengths)
        tri[1, 0] = (torch.rand(1, generator=g, dtype=torch.float64) - 0.5) * 0.6 * lengths[0]
        tri[2, 0] = (torch.rand(1, generator=g, dtype=torch.float64) - 0.5) * 0.6 * lengths[0]
        tri[2, 1] = (torch.rand(1, generator=g, dtype=torch.float64) - 0.5) * 0.6 * lengths[1]
        cell = tri @ _rotation(g)                       # all nine entries non-zero
        if k % 2 == 1:
            cell = cell[[1, 0, 2]]                      # left-handed: det < 0
        pbc = torch.rand(3, generator=g) < 0.6
        if not bool(pbc.any()):
            pbc[int(torch.randint(0, 3, (1,), generator=g))] = True
        kmax = 3
        if k in WRAPPED_FAR:
            n, pbc = WRAPPED_FAR[k][0], torch.tensor(WRAPPED_FAR[k][1])
            kmax = 50
        cell = cell.float()
        frac = torch.rand(n, 3, generator=g, dtype=torch.float64)
        frac = torch.where(pbc[None, :], frac, frac * 3.0 - 1.0)       # free axes: atoms also outside the cell
        R0 = (frac @ cell.double()).float()
        K = torch.randint(-kmax, kmax + 1, (n, 3), generator=g) * pbc[None, :].long()
        cutoff = float(2.0 + 3.5 * torch.rand(1, generator=g))
        out.append(("wrapped[%d]" % k, R0, K, cell, pbc, cutoff))
    return out


def wrapped():
    return [_one(name, R0.double() + K.double() @ cell.double(), cell, pbc, rc) for name, R0, K, cell, pbc, rc in wrapped_parts()]


def wrapped_in_cell():
    """The same systems before the displacement (R0); only the +-3 ones, for the metamorphic checks."""
    return [_one(name.replace("wrapped", "wrapped0"), R0, cell, pbc, rc)
            for k, (name, R0, K, cell, pbc, rc) in enumerate(wrapped_parts()) if k not in WRAPPED_FAR]


# ---------------------------------------------------------------------------------------------------------
# lattice: exact coordinates, pairs exactly at the cutoff
# ---------------------------------------------------------------------------------------------------------
CUT2_NEXT = float(np.nextafter(np.float32(2.0), np.float32(np.inf)))


def lattice():
    pts = torch.cartesian_prod(torch.arange(4.0), torch.arange(4.0), torch.arange(4.0))
    cell = torch.eye(3) * 4.0
    out = []
    for tag, shift in (("", (0.0, 0.0, 0.0)), ("_moved", (-8.0, 12.0, 4.0))):
        for kind, pbc in (("periodic", [True, True, True]), ("free", [False, False, False]), ("slab", [True, True, False])):
            for ctag, rc in (("2.0", 2.0), ("2.0+ulp", CUT2_NEXT)):
                out.append(_one("lattice[%s%s,%s]" % (kind, tag, ctag), pts + torch.tensor(shift), cell, pbc, rc))
    return out


# ---------------------------------------------------------------------------------------------------------
# dense: every atom of a system in one bin
# ---------------------------------------------------------------------------------------------------------
DENSE_COUNTS = [63, 64, 65, 127, 128, 129, 200]
DENSE_CUBE_SEEDS = {63: 3063, 64: 2064, 65: 2065, 127: 2127, 128: 7128, 129: 3129}     # 2000 + n, + 1000 t where that hit the band


def dense():
    out = []
    for n in DENSE_COUNTS:
        g = _gen(3000 + n)
        v = torch.randn(n, 3, generator=g, dtype=torch.float64)
        r = 1.5 * torch.rand(n, 1, generator=g, dtype=torch.float64) ** (1.0 / 3.0)
        out.append(_one("dense[blob,%d]" % n, v / torch.linalg.norm(v, dim=1, keepdim=True) * r, torch.zeros(3, 3), [False] * 3, 5.0))
    for n in DENSE_COUNTS[:-1]:
        g = _gen(DENSE_CUBE_SEEDS[n])
        out.append(_one("dense[cube,%d]" % n, torch.rand(n, 3, generator=g, dtype=torch.float64) * 4.0, torch.eye(3) * 4.0, [True] * 3, 5.0))
    return out


# ---------------------------------------------------------------------------------------------------------
# batches: many systems, empty ones included
# ---------------------------------------------------------------------------------------------------------
# 260 is the smallest batch after 257 whose second scan block of k_nbl_binoffsets (systems 256..) holds atoms in a
# system that would share bins with a populated one: with the last two systems empty, batches[257] has an empty system
# 256; in batches[260] system 257 has four atoms, and without the carry its bins are those of system 1
BATCH_SEEDS = {1: 4001, 255: 4255, 256: 4256, 257: 4257, 260: 4260, 600: 4600}


def _batch(name, n_sys, seed, trailing_unused=0):
    g = _gen(seed)
    counts = torch.randint(1, 5, (n_sys,), generator=g)
    counts[torch.rand(n_sys, generator=g) < 0.15] = 0
    if n_sys == 1:
        counts[0] = 3
    if n_sys >= 16:
        counts[0] = 0
        counts[7:10] = 0
        counts[-2:] = 0
        counts[1] = 4
        counts[-3] = 4
    cells = torch.zeros(n_sys, 3, 3)
    pbcs = torch.zeros(n_sys, 3, dtype=torch.bool)
    Rs = []
    for m in range(n_sys):
        L = 3.0 + 3.0 * torch.rand(3, generator=g, dtype=torch.float64)
        periodic = bool(torch.rand(1, generator=g) < 0.5)
        cells[m] = torch.diag(L).float()
        pbcs[m] = periodic
        Rs.append(torch.rand(int(counts[m]), 3, generator=g, dtype=torch.float64) * cells[m].double().diagonal())
    R = torch.cat(Rs).float()
    idx_m = torch.repeat_interleave(torch.arange(n_sys), counts)
    if trailing_unused:
        cells = torch.cat([cells, torch.eye(3).repeat(trailing_unused, 1, 1) * 5.0])
        pbcs = torch.cat([pbcs, torch.ones(trailing_unused, 3, dtype=torch.bool)])
    return (name, R, idx_m, cells, pbcs, 4.0)


def batches():
    out = [_batch("batches[%d]" % n, n, seed) for n, seed in BATCH_SEEDS.items()]
    out.append(_batch("batches[40+5unused]", 40, 4040, trailing_unused=5))     # n_systems > idx_m.max() + 1
    return out


# ---------------------------------------------------------------------------------------------------------
# sparse: fewer bins than the geometry allows
# ---------------------------------------------------------------------------------------------------------
def sparse():
    out = []
    R = torch.tensor([[0.5, 50.0, 50.0], [99.0, 50.5, 49.0],        # across the x face
                      [20.0, 0.25, 20.0], [21.0, 99.5, 20.5],       # across the y face
                      [70.0, 70.0, 99.5], [70.5, 71.0, 1.0],        # across the z face
                      [49.5, 50.5, 50.0]])                          # alone at the centre (a bin face of the unclipped grid)
    out.append(_one("sparse[cube100]", R, torch.eye(3) * 100.0, [True] * 3, 3.0))
    g = _gen(5001)
    c = torch.rand(20, 3, generator=g, dtype=torch.float64) * torch.tensor([200.0, 6.0, 6.0])
    d = torch.randn(20, 3, generator=g, dtype=torch.float64)
    d = d / torch.linalg.norm(d, dim=1, keepdim=True) * (1.0 + 1.5 * torch.rand(20, 1, generator=g, dtype=torch.float64))
    out.append(_one("sparse[rod200x6x6]", torch.cat([c, c + d]), torch.diag(torch.tensor([200.0, 6.0, 6.0])), [True] * 3, 3.0))
    g = _gen(5002)
    c = torch.rand(20, 3, generator=g, dtype=torch.float64) * torch.tensor([20.0, 20.0, 60.0])
    c[0, 2], c[1, 2] = 0.0, 60.0
    d = torch.randn(20, 3, generator=g, dtype=torch.float64)
    d = d / torch.linalg.norm(d, dim=1, keepdim=True) * (1.0 + 1.5 * torch.rand(20, 1, generator=g, dtype=torch.float64))
    d[:2, 2] = 0.0
    out.append(_one("sparse[slab20x20,z60]", torch.cat([c, c + d]), torch.diag(torch.tensor([20.0, 20.0, 90.0])), [True, True, False], 3.0))
    g = _gen(5003)
    x = torch.arange(6, dtype=torch.float64) * 15.6
    a = torch.stack([x, 0.3 * torch.rand(6, generator=g, dtype=torch.float64), 0.3 * torch.rand(6, generator=g, dtype=torch.float64)], 1)
    b = a + torch.tensor([2.0, 0.0, 0.0]) * (0.6 + 0.5 * torch.rand(6, 1, generator=g, dtype=torch.float64))
    b[-1, 0] = 80.0
    out.append(_one("sparse[chain80]", torch.cat([a, b]), torch.zeros(3, 3), [False] * 3, 3.0))
    return out


# ---------------------------------------------------------------------------------------------------------
# degenerate free geometry, single atoms, far from the origin
# ---------------------------------------------------------------------------------------------------------
def degenerate():
    out = []
    free = [False] * 3
    t = torch.tensor([0.0, 1.0, 2.5, 4.5, 9.0], dtype=torch.float64)
    out.append(_one("degenerate[collinear]", t[:, None] * torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64) + torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64), torch.zeros(3, 3), free, 3.0))
    out.append(_one("degenerate[coplanar]", torch.tensor([[0.0, 0, 0.5], [1.0, 0, 0.5], [0, 2.0, 0.5], [4.0, 4.0, 0.5], [4.5, 2.5, 0.5]]), torch.zeros(3, 3), free, 3.0))
    out.append(_one("degenerate[coincident]", torch.tensor([[1.25, -2.5, 3.0]]).repeat(5, 1), torch.zeros(3, 3), free, 3.0))
    out.append(_one("degenerate[one_atom_cube1.5]", torch.tensor([[0.4, 0.7, 1.1]]), torch.eye(3) * 1.5, [True] * 3, 6.0))
    tric = torch.tensor([[3.1, 0.0, 0.0], [1.0, 2.5, 0.0], [0.5, 2.0, 1.2]])           # heights: ..., ..., 1.2
    out.append(_one("degenerate[one_atom_height1.2]", torch.tensor([[0.3, 0.2, 0.1]]), tric, [True] * 3, 6.0))
    out.append(_one("degenerate[pair_through_shift]", torch.tensor([[0.5, 5.0, 5.0], [9.5, 5.25, 4.75]]), torch.eye(3) * 10.0, [True] * 3, 2.0))
    # fractional coordinate -1e-9: floor gives -1 and f - floor rounds to 1.0 in float32 (the g >= 1 fix-up of k_nbl_bin)
    out.append(_one("degenerate[frac_rounds_to_one]", torch.tensor([[-1.0e-8, 5.0, 5.0], [9.25, 5.0, 5.0], [0.75, 5.0, 5.0]]), torch.eye(3) * 10.0, [True] * 3, 2.0))
    g = _gen(6001)
    mol = torch.randn(21, 3, generator=g, dtype=torch.float64) * 2.0
    out.append(_one("degenerate[far_molecule]", mol + torch.tensor([1000.0, -2000.0, 500.0], dtype=torch.float64), torch.zeros(3, 3), free, 4.0))
    return out


# ---------------------------------------------------------------------------------------------------------
# md: the batch handed to NeighborListMD (bare cutoff 3.0), before and after one cell entry changed
# ---------------------------------------------------------------------------------------------------------
MD_SYSTEMS = (2, 20, 25)
MD_CUTOFF, MD_SHELL = 3.0, 0.5


def md():
    w = wrapped()
    parts = [w[k] for k in MD_SYSTEMS]
    R = torch.cat([p[1] for p in parts])
    idx_m = torch.repeat_interleave(torch.arange(len(parts)), torch.tensor([p[1].shape[0] for p in parts]))
    cells = torch.cat([p[3] for p in parts])
    pbcs = torch.cat([p[4] for p in parts])
    changed = cells.clone()
    changed[1, 0, 0] += 0.25
    return [("md[3systems]", R, idx_m, cells, pbcs, MD_CUTOFF), ("md[3systems,cell_changed]", R, idx_m, changed, pbcs, MD_CUTOFF)]


# d == cutoff exactly, in float32 and in float64 alike: integer lattice vectors of length 2, and the images of a
# single atom (R_j - R_i = 0, |S.cell| = 4 * 1.5)
EXACT_AT_CUTOFF = tuple(c[0] for c in lattice()) + ("degenerate[one_atom_cube1.5]",)

BUILDERS = {"wrapped": wrapped, "lattice": lattice, "dense": dense, "batches": batches, "sparse": sparse, "degenerate": degenerate, "md": md}


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(c for b in BUILDERS.values() for c in b())


def case_names():
    return [c[0] for c in all_cases()]


def case(name):
    return next(c for c in all_cases() + tuple(wrapped_in_cell()) if c[0] == name)


# ---------------------------------------------------------------------------------------------------------
# the reference of a case and its guard band
# ---------------------------------------------------------------------------------------------------------
def _distances(R, i, j, S, idx_m, cells):
    off = torch.einsum("ek,ekl->el", S.double(), cells.double()[idx_m[i]]) if i.numel() else torch.zeros(0, 3, dtype=torch.float64)
    return torch.linalg.norm(R.double()[j] - R.double()[i] + off, dim=1), off


@functools.lru_cache(maxsize=None)
def reference(name):
    """Oracle list of a case in canonical order (computed once per process, never modified):
    dict with idx_i, idx_j, S (int64), offsets (float64 S @ cell), d (float64 distances)."""
    _, R, idx_m, cells, pbcs, cutoff = case(name)
    i, j, S, off = NB.batch_neighbor_list(R.double(), idx_m, cells.double(), pbcs, cutoff, extra_repeats="auto", n_sys=cells.shape[0])
    order = NB.canonical_order(i, j, S)
    i, j, S, off = i[order], j[order], S[order], off[order]
    d, _ = _distances(R, i, j, S, idx_m, cells)
    return {"idx_i": i, "idx_j": j, "S": S, "offsets": off, "d": d}


@functools.lru_cache(maxsize=None)
def guard_band(name):
    """(band, distances of every pair within cutoff + an upper bound of the band).  The upper bound uses
    |S.cell| <= |R_j - R_i| + cutoff + band for any pair that close; the band itself then takes max|S.cell| of
    exactly those pairs."""
    _, R, idx_m, cells, pbcs, cutoff = case(name)
    rmax = float(torch.linalg.norm(R.double(), dim=1).max()) if R.shape[0] else 0.0
    ub = 16 * EPS32 * (rmax + (2.0 * rmax + 2.0 * cutoff) + cutoff)
    ub = ub / (1.0 - 16 * EPS32)
    i, j, S, _ = NB.batch_neighbor_list(R.double(), idx_m, cells.double(), pbcs, cutoff + ub, extra_repeats="auto", n_sys=cells.shape[0])
    d, off = _distances(R, i, j, S, idx_m, cells)
    omax = float(torch.linalg.norm(off, dim=1).max()) if off.shape[0] else 0.0
    band = 16 * EPS32 * (rmax + omax + cutoff)
    assert band <= ub
    return band, d


# ---------------------------------------------------------------------------------------------------------
# NumPy restatement of k_nbl_desc / k_nbl_bin (header comment of csrc/spk_nbl.hip): bins, reach, wraps
# ---------------------------------------------------------------------------------------------------------
def geometry(name):
    """Per system: nb_geom (bins the geometry allows), nb (after "never more bins than atoms"), reach, hb,
    occupancy (atoms in the fullest bin), wrap (integer cell wraps per atom), natoms.  float32 throughout."""
    _, R, idx_m, cells, pbcs, cutoff = case(name)
    f32 = np.float32
    rc = f32(cutoff)
    out = []
    for m in range(cells.shape[0]):
        Rm = R[idx_m == m].numpy().astype(f32)
        n = Rm.shape[0]
        pbc = pbcs[m].numpy()
        c = cells[m].numpy().astype(f32).reshape(9) if pbc.any() else np.eye(3, dtype=f32).reshape(9)
        idet = f32(1.0) / (c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]))
        inv = np.array([(c[4] * c[8] - c[5] * c[7]), (c[2] * c[7] - c[1] * c[8]), (c[1] * c[5] - c[2] * c[4]),
                        (c[5] * c[6] - c[3] * c[8]), (c[0] * c[8] - c[2] * c[6]), (c[2] * c[3] - c[0] * c[5]),
                        (c[3] * c[7] - c[4] * c[6]), (c[1] * c[6] - c[0] * c[7]), (c[0] * c[4] - c[1] * c[3])], dtype=f32).reshape(3, 3) * idet
        frac = (Rm @ inv).astype(f32) if n else np.zeros((0, 3), f32)
        h = f32(1.0) / np.sqrt((inv * inv).sum(0, dtype=f32))
        fmin, fext, H = np.zeros(3, f32), np.ones(3, f32), h.copy()
        for k in range(3):
            if not pbc[k]:
                lo, hi = (frac[:, k].min(), frac[:, k].max()) if n else (f32(0), f32(0))
                fmin[k], fext[k] = lo, max(hi - lo, f32(0))
                H[k] = fext[k] * h[k]
        nb_geom = [min(max(int(math.floor(H[k] / rc)), 1), 1024) for k in range(3)]
        nb = list(nb_geom)
        cap = max(n, 1)
        if nb[0] * nb[1] * nb[2] > cap:
            f = f32(np.cbrt(f32(cap) / f32(nb[0] * nb[1] * nb[2])))
            nb = [max(int(math.floor(f32(v) * f)), 1) for v in nb]
            while nb[0] * nb[1] * nb[2] > cap:
                kmax = (0 if nb[0] >= nb[2] else 2) if nb[0] >= nb[1] else (1 if nb[1] >= nb[2] else 2)
                nb[kmax] -= 1
        hb = [f32(H[k]) / f32(nb[k]) for k in range(3)]
        reach = []
        for k in range(3):
            r = int(math.ceil(rc / hb[k] * f32(1.0 + 1e-5))) if hb[k] > 0 else 0
            reach.append(min(r, nb[k] - 1) if not pbc[k] else r)
        wrap = np.zeros((n, 3), np.int64)
        fixups = 0
        bins = np.zeros((n, 3), np.int64)
        for k in range(3):
            if pbc[k]:
                fl = np.floor(frac[:, k])
                g = (frac[:, k] - fl).astype(f32)
                wrap[:, k] = fl.astype(np.int64) + (g >= 1)
                fixups += int((g >= 1).sum())
                g = np.where(g >= 1, f32(0), g)
            else:
                g = (frac[:, k] - fmin[k]) / fext[k] if fext[k] > 0 else np.zeros(n, f32)
            bins[:, k] = np.clip((g * f32(nb[k])).astype(np.int64), 0, nb[k] - 1)
        flat = (bins[:, 0] * nb[1] + bins[:, 1]) * nb[2] + bins[:, 2]
        occ = int(np.bincount(flat).max()) if n else 0
        out.append({"natoms": n, "nb_geom": nb_geom, "nb": nb, "reach": reach, "hb": hb, "occupancy": occ, "wrap": wrap,
                    "fixups": fixups, "frac": frac, "det": float(1.0 / idet), "fext": fext, "pbc": pbc})
    return out
