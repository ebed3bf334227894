"""Molecule layouts, seeded inputs, the float64 formula, the dispatch predicate and the error measure for the Atomwise head kernels
(csrc/spk_dense.hip: k_atomwise_fwd16 on 16-atom tiles, k_atomwise_fwd on 32-atom tiles in workgroups of 128 atoms, k_atomwise_bwd on
32 x 32 tiles; dispatch in spk_atomwise_fwd_f32).  Shared by tests/test_atomwise_head_cases.py (CPU: every layout has the property its
name claims, the formula agrees with autograd on an independent formulation, and the same formula in float32 on the host stays below
half the device bound) and tests/test_gpu_atomwise_head.py.  Plain torch, no fixtures, every draw seeded.

The head:  pre_n = W1 x_n + b1,  y_n = w2 . act(pre_n) + b2,  E[idx_m[n]] += y_n,  and for L = sum wE . E + sum wA . y:
dL/dx_n = s_n (w2 * act'(pre_n)) W1  with  s_n = wE[idx_m[n]] + wA[n].  Nothing in the operator asks for an ascending idx_m.

Both forward kernels keep the molecule sums of a workgroup in 128 LDS slots relative to the molecule of the workgroup's first atom
(rel = mol - mol0) and send every other molecule straight to a global atomic; the layouts below reach rel < 0 (`descending`),
rel >= 128 (`far`, `each` across a 128-atom block), several segments of one tile on one slot (`interleaved`) and all 128 slots (`each`).
"""
import functools
import math

import torch

TILE16, TILE32, BLOCK32, SLOTS = 16, 32, 128, 128
LAYOUTS = ("one", "each", "ragged", "gaps", "interleaved", "descending", "far")
ACTS = ("silu", "ssp")
ACT_ID = {"ssp": 1, "silu": 2}                       # SPK_ACT_SSP, SPK_ACT_SILU of include/spk_hip.h

FWD16_SHAPES = ((32, 32), (64, 32), (128, 64), (512, 64))          # (n_in, n_hidden) the 16-atom kernel takes
FWD32_SHAPES = ((544, 64), (128, 96), (192, 128), (128, 160))      # ... and the first widths that leave it
TILE_NS = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129)
TILE_LAYOUTS = ("one", "ragged", "gaps", "interleaved")
EDGE_SHAPE = (128, 64)
EDGE_LAYOUTS = ("one", "each", "interleaved", "far")
BWD_SHAPES = ((32, 32), (128, 64), (544, 64), (128, 96), (128, 160))
BWD_NS = (1, 31, 32, 33, 129)
BWD_LAYOUTS = ("ragged", "gaps", "interleaved")
BWD_MODES = ("gE", "gy", "both")


def edge_ns(n_cu):
    """The largest atom count the 16-atom kernel takes on a device of n_cu compute units, and the first the 32-atom kernel takes."""
    return (32 * n_cu, 32 * n_cu + 1)


def both_kernel_ns(n_cu):
    return (17, 129, 32 * n_cu)


def takes_fwd16(n_in, H, N, n_cu, b1_aligned=True, simple=False):
    """The dispatch predicate of spk_atomwise_fwd_f32, restated: True when the call runs k_atomwise_fwd16 (an absent b1 counts as aligned)."""
    return H in (32, 64) and n_in <= 512 and bool(b1_aligned) and not simple and (N + TILE16 - 1) // TILE16 <= 2 * n_cu


def block_starts(kernel, N, n_cu):
    """First atom of every workgroup's contiguous range: 128 atoms in the 32-atom kernel (its grid-stride loop walks such blocks), a
    share of the 16-atom tiles in the 16-atom kernel (tiles_per_block of the launcher)."""
    if kernel == "fwd32":
        return list(range(0, N, BLOCK32))
    nt = (N + TILE16 - 1) // TILE16
    nblk = min(nt, 2 * n_cu)
    tpb = (nt + nblk - 1) // nblk
    return list(range(0, N, TILE16 * tpb))


# ---------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------
def _sizes(N, largest, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    sizes, left = [], N
    while left > 0:
        s = min(left, int(torch.randint(1, largest + 1, (1,), generator=g)))
        sizes.append(s)
        left -= s
    return sizes


def _ascending(N, largest, seed):
    sizes = _sizes(N, largest, seed)
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.int64)), len(sizes)


@functools.lru_cache(maxsize=None)
def layout(name, N, seed=0):
    """(idx_m int64 [N], n_mol); every id lies in [0, n_mol).

    one          all atoms in molecule 0
    each         idx_m = arange(N): 128 distinct ids per 128 atoms, rel >= 128 from the second tile pair of a 32-atom workgroup's block on
    ragged       ascending, sizes drawn from 1 ... 39
    gaps         ascending runs of 1 ... 5 atoms on the ids 1, 4, 5, 9, 12, 13, 17 ... (steps 3, 1, 4 repeated); n_mol = largest id + 4: ids
                 without atoms at the front, inside and at the end
    interleaved  arange(N) % 3 with n_mol = 3: every atom its own segment, every full tile holds each molecule in five segments
    descending   `ragged` reversed: rel < 0 for every molecule but the first of a workgroup
    far          `ragged`, except that the last atom of every full 16-atom tile belongs to molecule n_mol - 1; n_mol is the ragged count + 200
                 for N >= 200 (+ 1 below), so that molecule is at least 128 ids past every workgroup's first and the ids between hold nothing
    """
    assert N >= 0
    if name == "one":
        return torch.zeros(N, dtype=torch.int64), 1
    if name == "each":
        return torch.arange(N, dtype=torch.int64), max(N, 1)
    if name == "ragged":
        idx, nm = _ascending(N, 39, seed)
        return idx, max(nm, 1)
    if name == "gaps":
        runs, nm = _ascending(N, 5, seed + 1)
        steps = torch.tensor([3, 1, 4], dtype=torch.int64)
        ids = 1 + torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(steps.repeat(nm // 3 + 1), 0)])[:max(nm, 1)]
        return (ids[runs] if N else runs), int(ids[max(nm, 1) - 1]) + 4
    if name == "interleaved":
        return torch.arange(N, dtype=torch.int64) % 3, 3
    if name == "descending":
        idx, nm = layout("ragged", N, seed)
        return torch.flip(idx, [0]), nm
    if name == "far":
        idx, nm = layout("ragged", N, seed)
        n_mol = nm + (200 if N >= 200 else 1)
        idx = idx.clone()
        idx[TILE16 - 1::TILE16] = n_mol - 1
        return idx, n_mol
    raise KeyError(name)


def segments(ids):
    """Runs of equal id in a 1-d tensor: list of (id, length)."""
    out = []
    for v in ids.tolist():
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return [(a, b) for a, b in out]


# ---------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------
def _f32(t):
    return t.float().double()


@functools.lru_cache(maxsize=64)
def _drawn(n_in, H, N, seed):
    g = torch.Generator().manual_seed(7919 * seed + 31 * n_in + 17 * H + N)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return {"x": _f32(r(N, n_in)), "w1": _f32(r(H, n_in) / math.sqrt(n_in)), "b1": _f32(0.3 * r(H)), "w2": _f32(r(H) / math.sqrt(H)),
            "b2": _f32(torch.full((1,), 0.5, dtype=torch.float64)), "wA": _f32(r(N))}


def head_inputs(n_in, H, N, seed=0, n_mol=1):
    """x ~ N(0, 1) [N, n_in], w1 ~ N(0, 1) / sqrt(n_in) [H, n_in], b1 ~ 0.3 N(0, 1) [H], w2 ~ N(0, 1) / sqrt(H) [H], b2 = 0.5 [1] (a non-zero mean
    keeps molecule sums from cancelling: max|E| is a fair scale), upstream weights wE ~ N(0, 1) [n_mol] and wA ~ N(0, 1) [N]; all rounded to
    float32 and held in float64.  x, the parameters and wA depend on (n_in, H, N, seed) alone, so every layout of a shape sees the same head."""
    d = dict(_drawn(n_in, H, N, seed))
    g = torch.Generator().manual_seed(104729 * seed + 13 * n_mol + N)
    d["wE"] = _f32(torch.randn(n_mol, generator=g, dtype=torch.float64))
    return d


def make_case(n_in, H, N, name, seed=0):
    idx_m, n_mol = layout(name, N, seed)
    c = head_inputs(n_in, H, N, seed, n_mol)
    c.update(idx_m=idx_m, n_mol=n_mol, n_in=n_in, H=H, N=N, layout=name, seed=seed,
             label="%dx%d N=%d %s" % (n_in, H, N, name))
    return c


def empty_ids(c):
    """Molecule ids in [0, n_mol) that no atom carries."""
    has = torch.zeros(c["n_mol"], dtype=torch.bool)
    has[c["idx_m"]] = True
    return (~has).nonzero().flatten()


# ---------------------------------------------------------------------------------------------------------
# the formula
# ---------------------------------------------------------------------------------------------------------
LN2 = math.log(2.0)


def act_fn(act, v):
    if act == "silu":
        return v * torch.sigmoid(v)
    if act == "ssp":
        return torch.nn.functional.softplus(v) - LN2
    raise KeyError(act)


def act_grad(act, v):
    s = torch.sigmoid(v)
    if act == "silu":
        return s * (1 + v * (1 - s))
    if act == "ssp":
        return s
    raise KeyError(act)


def head_formula(c, act, dtype=torch.float64, b1=True, b2=True, use_gE=True, use_gy=True):
    """pre [N, H], y_atom [N], E [n_mol], gx [N, n_in] of the head in `dtype`, by the closed formulas of the module docstring (no autograd);
    the molecule sum is index_add_, which takes any order of idx_m.  b1 / b2 = False: the head without that bias; use_gE / use_gy = False:
    the gradient without that upstream term."""
    x, w1, w2 = c["x"].to(dtype), c["w1"].to(dtype), c["w2"].to(dtype)
    pre = x @ w1.T
    if b1:
        pre = pre + c["b1"].to(dtype)
    y = act_fn(act, pre) @ w2
    if b2:
        y = y + c["b2"].to(dtype)
    E = torch.zeros(c["n_mol"], dtype=dtype).index_add_(0, c["idx_m"], y)
    s = torch.zeros(c["N"], dtype=dtype)
    if use_gE:
        s = s + c["wE"].to(dtype)[c["idx_m"]]
    if use_gy:
        s = s + c["wA"].to(dtype)
    gx = (s[:, None] * w2[None, :] * act_grad(act, pre)) @ w1
    return {"pre": pre, "y_atom": y, "E": E, "gx": gx}


def head_ref(c, act, **kw):
    """The float64 oracle."""
    return head_formula(c, act, torch.float64, **kw)


def rel(a, b):
    """max|a - b| / max|b|, the project's measure (the absolute error where the reference is identically 0)."""
    b = b.double()
    m = float(b.abs().max()) if b.numel() else 0.0
    e = float((a.double() - b).abs().max()) if b.numel() else 0.0
    return e / m if m > 0 else e


# ---------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_atomwise_head.py, for the conditioning test
# ---------------------------------------------------------------------------------------------------------
def gpu_cases(n_cu):
    """Every (n_in, H, N, layout) the GPU file runs on a device of n_cu compute units, each once."""
    seen, out = set(), []

    def add(shape, N, name):
        k = (shape[0], shape[1], N, name)
        if k not in seen:
            seen.add(k)
            out.append(k)
    for shape in FWD16_SHAPES + FWD32_SHAPES:
        for N in TILE_NS:
            for name in TILE_LAYOUTS:
                add(shape, N, name)
    for N in edge_ns(n_cu):
        for name in EDGE_LAYOUTS:
            add(EDGE_SHAPE, N, name)
    for shape in FWD16_SHAPES:
        for N in both_kernel_ns(n_cu):
            for name in LAYOUTS:
                add(shape, N, name)
    for shape in BWD_SHAPES:
        for N in BWD_NS:
            for name in BWD_LAYOUTS:
                add(shape, N, name)
    for N in (33, 129, 32 * n_cu + 1):
        for name in ("interleaved", "gaps"):
            add(EDGE_SHAPE, N, name)
    return out
