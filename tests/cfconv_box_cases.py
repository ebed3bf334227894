"""Seeded neighbour lists on the row and tile edges of the general-list SchNet kernels (csrc/spk_cfconv.hip): the row-tile forward
works through a row in chunks of 32 edges with a wavefront per row and 16 rows per workgroup, the pair kernels through the list of
canonical pairs (``half``: the edges with idx_i < idx_j, in list order) in tiles of 32, and both walk their work XCD-contiguously on
large lists.  Shared by tests/test_cfconv_box_cases.py (CPU: every case has the properties its docstring states, and the same formula in
float32 on the host is well inside the bounds) and tests/test_gpu_cfconv_box.py.  Plain numpy / torch, no fixtures, every draw seeded.

Every list gives its pair vectors directly (no positions), antisymmetric on the symmetric lists, with ``idx_i`` ascending and
``idx_j`` ascending within a row.  A case is a dict: N, idx_i, idx_j, r_ij (torch, float32 / int64) and ``info``.

Lengths.  A row whose ONLY pair lies close to the cutoff is ill-conditioned by itself in float32, whatever the kernel: f_c =
(cos(pi d / r_c) + 1) / 2 carries an absolute error of ~1e-7, which is 1e-5 of the row as soon as f_c < 0.01 (d > 4.68 A).  Pairs that
are the only pair of a row (dimers, the spokes of a star) therefore have d < ``D_SINGLE`` = 4 A (f_c > 0.095) or lie beyond the
cutoff; rows with many pairs take the whole range, since their near pairs carry the scale.
"""
import functools

import numpy as np
import torch

from oracle import spk_oracle as O

CUTOFF, TILE, ROW_WAVES, NF = 5.0, 32, 16, 128
D_SINGLE = 4.0
ROW_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 96, 97)
BASES = ((8, "gaussian"), (13, "gaussian"), (16, "gaussian"), (20, "gaussian"), (32, "gaussian"), (13, "bessel"), (20, "bessel"))
CLIQUES = (32, 33, 34, 64, 65, 66, 97, 98)          # row lengths n - 1
STARS = (64, 33)                                      # spokes; the centre is the FIRST atom: its run in `half` starts a tile


# ---------------------------------------------------------------------------------------------------------
# structure
# ---------------------------------------------------------------------------------------------------------
def _structure(n_dimers, iso=(2, 3, 2)):
    """Undirected pairs (a < b) of: `iso[0]` isolated atoms, the stars, half of the cliques, `iso[1]` isolated atoms, the other
    cliques, the dimers, `iso[2]` isolated atoms.  Returns (N, a, b, kind) with kind 0 = pair of a long row on both sides (clique),
    1 = the only pair of some row (spoke, dimer), and the ring pairs of every clique (k, k + 1) flagged 2."""
    a, b, kind = [], [], []
    n = iso[0]
    for k in STARS:
        a += [n] * k; b += list(range(n + 1, n + 1 + k)); kind += [1] * k
        n += k + 1
    for q, c in enumerate(CLIQUES):
        if q == len(CLIQUES) // 2:
            n += iso[1]
        for u in range(c):
            for v in range(u + 1, c):
                a.append(n + u); b.append(n + v); kind.append(2 if (v == u + 1 or (u == 0 and v == c - 1)) else 0)
        n += c
    for _ in range(n_dimers):
        a.append(n); b.append(n + 1); kind.append(1)
        n += 2
    n += iso[2]
    return n, np.array(a, dtype=np.int64), np.array(b, dtype=np.int64), np.array(kind)


def _base_pairs():
    return int(sum(STARS) + sum(c * (c - 1) // 2 for c in CLIQUES))


def _directed(N, a, b, v):
    """Both directions of the pairs (a < b) with vectors v (a -> b), sorted by (idx_i, idx_j), as torch arrays."""
    ii, jj = np.concatenate([a, b]), np.concatenate([b, a])
    r = np.concatenate([v, -v]).astype(np.float32)
    order = np.lexsort((jj, ii))
    return {"N": int(N), "idx_i": torch.from_numpy(ii[order]), "idx_j": torch.from_numpy(jj[order]),
            "r_ij": torch.from_numpy(np.ascontiguousarray(r[order]))}


def _unit(rng, n):
    u = rng.randn(n, 3)
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _tail_dimers(last_tile):
    """Dimers (2 ... 33 of them, so that row length 1 occurs) that leave `last_tile` pairs in the last 32-pair tile."""
    want = last_tile % TILE
    k = (want - _base_pairs()) % TILE
    return k if k >= 2 else k + TILE


@functools.lru_cache(maxsize=None)
def rows(last_tile=1):
    """Cliques, stars, dimers and isolated atoms, every pair inside the cutoff (0.9 ... 4.9 A).  `last_tile` in (1, 32): pairs in
    the last tile of `half`."""
    rng = np.random.RandomState(100 + last_tile)
    iso = (2, 3, 2)
    N, a, b, kind = _structure(_tail_dimers(last_tile), iso)
    if N % ROW_WAVES == 0:
        iso = (2, 3, 3)
        N, a, b, kind = _structure(_tail_dimers(last_tile), iso)
    d = np.where(kind == 1, rng.uniform(0.9, D_SINGLE, len(a)), rng.uniform(0.9, 4.9, len(a)))
    c = _directed(N, a, b, _unit(rng, len(a)) * d[:, None])
    c["info"] = {"name": "rows_last%d" % last_tile, "iso": iso, "last_tile": last_tile}
    return c


@functools.lru_cache(maxsize=None)
def cutoff(live=None):
    """The structure of rows(1) with lengths uniform in (0.9, 1.12 x cutoff): the ring pairs of every clique lie beyond the cutoff, so
    every row of a clique holds pairs on both sides of it; a quarter of the spokes and dimers lie beyond it too.  Two chords of the
    largest clique are special: one pair with d == cutoff exactly in float32, one at nextafter(cutoff, 0) (axis-parallel vectors:
    the float32 norm is exact with or without fused multiply-adds).  live = None: as drawn; 0 / 1: pairs are pushed out until the
    count of canonical pairs inside the cutoff is 32 k / 32 k + 1; "none": every pair beyond the cutoff."""
    rng = np.random.RandomState(200)
    N, a, b, kind = _structure(_tail_dimers(1))
    if N % ROW_WAVES == 0:
        N, a, b, kind = _structure(_tail_dimers(1), (2, 3, 3))
    n = len(a)
    far = rng.uniform(1.01 * CUTOFF, 1.12 * CUTOFF, n)
    d = rng.uniform(0.9, 1.12 * CUTOFF, n)
    while True:                              # no drawn length within 1e-4 of the cutoff: inside / beyond is the same in every arithmetic
        near = np.abs(d - CUTOFF) < 1e-4
        if not near.any():
            break
        d[near] = rng.uniform(0.9, 1.12 * CUTOFF, int(near.sum()))
    single = np.where(rng.rand(n) < 0.25, far, rng.uniform(0.9, D_SINGLE, n))
    d = np.where(kind == 1, single, np.where(kind == 2, far, d))
    v = (_unit(rng, n) * d[:, None]).astype(np.float32)
    # the two special chords: atoms (0, 2) and (1, 3) of the last (largest) clique
    c0 = int(a[kind != 1][-1]) - (CLIQUES[-1] - 2)         # first atom of the last clique (its last pair is (c0 + n - 2, c0 + n - 1))
    at = np.nonzero((a == c0) & (b == c0 + 2))[0][0]
    below = np.nonzero((a == c0 + 1) & (b == c0 + 3))[0][0]
    v[at] = (0.0, np.float32(CUTOFF), 0.0)
    v[below] = (np.nextafter(np.float32(CUTOFF), np.float32(0.0)), 0.0, 0.0)
    special = np.zeros(n, dtype=bool); special[[at, below]] = True
    d32 = _norm32(v)
    if live == "none":
        scale = (far / np.maximum(d32, 1e-6)).astype(np.float32)
        v = np.where((d32 < CUTOFF)[:, None], v * scale[:, None], v).astype(np.float32)
    elif live is not None:
        inside = np.nonzero((d32 < CUTOFF) & ~special & (kind == 0))[0]
        k = (int((d32 < CUTOFF).sum()) - int(live)) % TILE
        out = inside[-k:] if k else inside[:0]
        v[out] = (v[out] * (far[out] / d32[out])[:, None]).astype(np.float32)
    c = _directed(N, a, b, v)
    c["info"] = {"name": "cutoff_%s" % ("drawn" if live is None else live), "exact_pair": (c0, c0 + 2), "below_pair": (c0 + 1, c0 + 3), "live": live}
    return c


def _norm32(v):
    v = np.asarray(v, dtype=np.float32)
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).astype(np.float32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def asymmetric():
    """A sorted, asymmetric list (as synthetic.random_graph_batch(sort=True), with distinct neighbours in a row): out-degrees cycle
    through 0 ... 40 around the chunk size, four hub atoms are the neighbour of almost every row and the last ten atoms of no row, so that the
    by-neighbour rows include lengths 0 and lengths far above 32.  Lengths in 0.8 ... 6 A as in random_graph_batch, except for a pair that
    is the only one of its row or of its by-neighbour row (module docstring)."""
    rng = np.random.RandomState(300)
    N = 203
    deg = np.array([0, 1, 5, 31, 32, 33, 40, 9, 64, 65])[np.arange(N) % 10]
    w = np.ones(N); w[:4] = 40.0; w[N - 10:] = 0.0
    ii, jj = [], []
    for i in range(N):
        p = w.copy(); p[i] = 0.0
        j = np.sort(rng.choice(N, size=int(deg[i]), replace=False, p=p / p.sum()))
        ii += [i] * len(j); jj += j.tolist()
    E = len(ii)
    d = rng.uniform(0.8, 6.0, E)
    ii_, jj_ = np.array(ii), np.array(jj)
    alone = (np.bincount(ii_, minlength=N)[ii_] == 1) | (np.bincount(jj_, minlength=N)[jj_] == 1)     # the only pair of a row, either way
    d = np.where(alone, np.where(rng.rand(E) < 0.25, rng.uniform(1.01 * CUTOFF, 6.0, E), rng.uniform(0.8, D_SINGLE, E)), d)
    v = (_unit(rng, E) * d[:, None]).astype(np.float32)
    return {"N": N, "idx_i": torch.tensor(ii, dtype=torch.int64), "idx_j": torch.tensor(jj, dtype=torch.int64), "r_ij": torch.from_numpy(v),
            "info": {"name": "asymmetric"}}


def walk_shape(compute_units):
    """(N, degree, conditions) of the ring list on which both XCD-contiguous walks are live on a device of `compute_units`."""
    N = 1 << 14
    while N % 8 == 0 or N % 16 == 0:
        N += 1
    degree = 2
    while True:
        tiles = -(-(N * degree // 2) // TILE)
        grid = min(compute_units, -(-tiles // 8))
        if tiles >= 16 * grid and tiles % 8 != 0:
            break
        degree += 2
    row_grid = min(compute_units, -(-N // ROW_WAVES))
    cond = {"N": N, "degree": degree, "tiles": tiles, "pair_grid": grid, "row_grid": row_grid,
            "n_at_least_2_14": N >= (1 << 14), "n_not_multiple_of_8": N % 8 != 0,
            "tiles_at_least_16_per_workgroup": tiles >= 16 * grid, "tiles_not_multiple_of_8": tiles % 8 != 0,
            "pair_walk_live": grid % 8 == 0 and tiles >= 16 * grid, "row_walk_live": row_grid % 8 == 0 and N >= (1 << 14)}
    return N, degree, cond


@functools.lru_cache(maxsize=None)
def walk(compute_units=256):
    from schnetpack_amd import synthetic as S
    N, degree, cond = walk_shape(compute_units)
    b = S.ring_graph_batch(N, degree, seed=400, dmin=0.9, dmax=4.9)
    return {"N": N, "idx_i": b["idx_i"], "idx_j": b["idx_j"], "r_ij": b["r_ij"], "info": dict(cond, name="walk")}


# ---------------------------------------------------------------------------------------------------------
# derived quantities of a list
# ---------------------------------------------------------------------------------------------------------
def row_lengths(c, by="idx_i"):
    return np.bincount(c[by].numpy(), minlength=c["N"])


def canonical(c):
    """Edges of the canonical pairs (idx_i < idx_j) in list order: the plan's `half` on a sorted symmetric list."""
    return np.nonzero((c["idx_i"] < c["idx_j"]).numpy())[0]


def half_runs(c):
    """(start, end) positions in `half` of every run of equal centre atom."""
    ci = c["idx_i"].numpy()[canonical(c)]
    cut = np.nonzero(np.diff(ci))[0] + 1
    return np.concatenate([[0], cut]), np.concatenate([cut, [len(ci)]])


def d32(c):
    """float32 lengths of the pair vectors, as the device computes them."""
    return _norm32(c["r_ij"].numpy())


def live_pairs(c):
    """Canonical pairs with d < cutoff, order kept: the per-call compacted list."""
    h = canonical(c)
    return h[d32(c)[h] < np.float32(CUTOFF)]


def reverse_edges(c):
    """rev[e]: the edge (j, i) of the edge e = (i, j) of a symmetric list."""
    key = c["idx_i"].numpy() * c["N"] + c["idx_j"].numpy()
    rkey = c["idx_j"].numpy() * c["N"] + c["idx_i"].numpy()
    pos = np.searchsorted(key, rkey)
    assert (key[pos] == rkey).all()
    return pos


# ---------------------------------------------------------------------------------------------------------
# parameters and inputs
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def filter_params(n_rbf, seed=3):
    """Filter network with non-zero biases (as _filter_params of tests/test_gpu_ops.py)."""
    g = torch.Generator().manual_seed(seed)
    return {"n_rbf": n_rbf, "w1": torch.randn(NF, n_rbf, generator=g) * 0.4, "b1": torch.randn(NF, generator=g) * 0.2,
            "w2": torch.randn(NF, NF, generator=g) / NF ** 0.5, "b2": torch.randn(NF, generator=g) * 0.2}


def features(N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, NF, generator=g), torch.randn(N, NF, generator=g)


@functools.lru_cache(maxsize=None)
def model_params(n_rbf, radial, n_layers):
    """Seeded SchNet representation (oracle names) whose filter networks have biases."""
    rep = O.init_schnet_params(NF, n_layers, n_rbf, CUTOFF, radial=radial)
    gen = torch.Generator().manual_seed(5)
    for l in range(n_layers):
        for k in (0, 1):
            rep["interactions.%d.filter_network.%d.bias" % (l, k)] = 0.2 * torch.randn(NF, generator=gen)
    return rep


def radial_params(n_rbf, radial):
    if radial == "gaussian":
        return O.gaussian_rbf_params(n_rbf, CUTOFF)
    return (O.bessel_rbf_params(n_rbf, CUTOFF).float(),)


# ---------------------------------------------------------------------------------------------------------
# the formula, in row blocks
# ---------------------------------------------------------------------------------------------------------
def _basis(d, n_rbf, radial, dtype):
    if radial == "gaussian":
        off, w = O.gaussian_rbf_params(n_rbf, CUTOFF)
        return O.gaussian_rbf(d, off.to(dtype), w.to(dtype))
    return O.bessel_rbf(d, O.bessel_rbf_params(n_rbf, CUTOFF).float().to(dtype))


def filter_rows(d, p, radial, dtype=torch.float64):
    """Raw filter W2 ssp(W1 phi(d) + b1) + b2 of every distance (no cutoff factor)."""
    z = O.dense(_basis(d.to(dtype), p["n_rbf"], radial, dtype), p["w1"].to(dtype), p["b1"].to(dtype), O.shifted_softplus)
    return O.dense(z, p["w2"].to(dtype), p["b2"].to(dtype))


def cfconv_ref(c, h, p, radial, gy=None, dtype=torch.float64, block=1 << 15):
    """y[i] = sum_e W_e o h[j(e)], W_e = filter(d_e) f_c(d_e) -- the formula of _cfconv_oracle (tests/test_gpu_ops.py), evaluated over blocks
    of `block` edges so that no [E, 128] tensor of the whole list is held.  Returns y and scale_y[i] = max_c sum_e |W_e o h_j| (the
    sum of absolute contributions of the row); with gy also gh[j] = sum_e W_e o gy[i(e)], its scale and gr = d<y, gy>/dr."""
    N, ii, jj = c["N"], c["idx_i"], c["idx_j"]
    h = h.to(dtype)
    r_all = c["r_ij"].to(dtype)
    y, ay = torch.zeros(N, NF, dtype=dtype), torch.zeros(N, NF, dtype=dtype)
    out = {}
    if gy is not None:
        gy = gy.to(dtype)
        gh, agh, gr = torch.zeros(N, NF, dtype=dtype), torch.zeros(N, NF, dtype=dtype), torch.zeros(len(ii), 3, dtype=dtype)
    for e0 in range(0, len(ii), block):
        sl = slice(e0, min(e0 + block, len(ii)))
        r = r_all[sl].clone().requires_grad_(gy is not None)
        d = torch.sqrt((r * r).sum(1))
        W = filter_rows(d, p, radial, dtype) * O.cosine_cutoff(d, CUTOFF)[:, None]
        m = h[jj[sl]] * W
        y.index_add_(0, ii[sl], m.detach())
        ay.index_add_(0, ii[sl], m.detach().abs())
        if gy is not None:
            t = gy[ii[sl]] * W
            gh.index_add_(0, jj[sl], t.detach())
            agh.index_add_(0, jj[sl], t.detach().abs())
            gr[sl] = torch.autograd.grad((m * gy[ii[sl]]).sum(), r)[0]
    out["y"], out["scale_y"] = y, ay.amax(1)
    if gy is not None:
        out["gh"], out["scale_gh"], out["gr"] = gh, agh.amax(1), gr
    return out


def representation_ref(c, x0, rep, n_layers, radial, gx_out=None, dtype=torch.float64, block=1 << 15):
    """x_out of the n_layers-interaction SchNet representation started from the features x0 (representation/schnet.py:147-173 after the
    embedding), the cfconv of every interaction through cfconv_ref; with gx_out also gr = d<x_out, gx_out>/dr_ij and gx0."""
    P = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in rep.items()}
    n_rbf = int((P["radial_basis.offsets"] if radial == "gaussian" else P["radial_basis.freqs"]).shape[0])
    fp = lambda l: {"n_rbf": n_rbf, "w1": P["interactions.%d.filter_network.0.weight" % l], "b1": P["interactions.%d.filter_network.0.bias" % l],
                    "w2": P["interactions.%d.filter_network.1.weight" % l], "b2": P["interactions.%d.filter_network.1.bias" % l]}
    x = x0.to(dtype)
    keep = []
    for l in range(n_layers):
        pre = "interactions.%d." % l
        h = O.dense(x, P[pre + "in2f.weight"])
        y = cfconv_ref(c, h, fp(l), radial, dtype=dtype, block=block)["y"].requires_grad_(gx_out is not None)
        v = O.dense(O.dense(y, P[pre + "f2out.0.weight"], P[pre + "f2out.0.bias"], O.shifted_softplus), P[pre + "f2out.1.weight"], P[pre + "f2out.1.bias"])
        keep.append((h, y, v))
        x = x + v.detach()
    out = {"x_out": x}
    if gx_out is not None:
        gx, gr = gx_out.to(dtype), torch.zeros(len(c["idx_i"]), 3, dtype=dtype)
        for l in reversed(range(n_layers)):
            h, y, v = keep[l]
            gy = torch.autograd.grad(v, y, gx)[0]
            b = cfconv_ref(c, h, fp(l), radial, gy=gy, dtype=dtype, block=block)
            gr += b["gr"]
            gx = gx + b["gh"] @ P["interactions.%d.in2f.weight" % l]
        out["gr"], out["gx0"] = gr, gx
    return out


# ---------------------------------------------------------------------------------------------------------
# error measures
# ---------------------------------------------------------------------------------------------------------
def max_norm_err(got, ref):
    ref = ref.double()
    m = float(ref.abs().max())
    e = float((got.double() - ref).abs().max())
    return e / m if m > 0 else e


def per_row_err(got, ref, scale):
    """max over the rows with scale > 0 of max_c |got - ref| / scale[row]; rows with scale == 0 (no pair inside the cutoff) must be exactly 0:
    returns (worst figure, its row, rows of scale 0 that are not exactly 0)."""
    diff = (got.double() - ref.double()).abs().amax(1)
    live = scale > 0
    fig = torch.where(live, diff / torch.where(live, scale, torch.ones_like(scale)), torch.zeros_like(diff))
    dead_bad = ((~live) & (got.double().abs().amax(1) != 0)).nonzero().flatten().tolist()
    row = int(fig.argmax())
    return float(fig[row]), row, dead_bad
