"""Seeded neighbour lists, inputs, the float64 formula and the error measures for the box-regime PaiNN message kernels
(csrc/spk_painn_tile.hip, dispatch in csrc/spk_painn.hip): the row-tile forward and backward walk a row in chunks of 32 pairs with a
wavefront per row and 4 rows per workgroup, the MFMA tile kernels walk the whole list in tiles of 32 edges, the row kernel in chunks of
64, and all of them walk their work XCD-contiguously on large lists.  Shared by tests/test_painn_box_cases.py (CPU: every case has the
properties its docstring states, and the same formula in float32 on the host is well inside the bounds) and
tests/test_gpu_painn_box.py.  Plain numpy / torch, no fixtures, every draw seeded.

Lists.  ``rows``, ``cutoff`` and ``asymmetric`` are those of tests/cfconv_box_cases.py (rows of 0, 1, 31 ... 33, 63 ... 65, 96, 97
pairs -- 34 and 66 are added by ``hubs`` --, stars, dimers, isolated atoms, a pair at d == cutoff and one at nextafter(cutoff, 0), canonical live counts 32 k, 32 k + 1 and
0; a pair that is the only one of its row has d < ``D_SINGLE`` or lies beyond the cutoff -- see that module's docstring).  New here:
``hubs`` (rows on both sides of RT_LIVE_CAP = 256, the longest row whose live pairs the skin instances compact) and ``walk`` (both
XCD-contiguous walks with a ragged last eighth).

Inputs.  c, gq ~ N(0, 1); the filter wf ~ 0.3 N(0, 1) with bias bf ~ 0.1 N(0, 1).  q, mu and gmu are drawn with standard deviation
``RESIDUAL`` = 0.25, not 1: the outputs q_out = q + dq, mu_out = mu + dmu, gmu_in = gmu_out + (sum) are measured per row AFTER the input
term is taken out, against the row's own sum of absolute contributions.  The rounding of that one addition is half an ulp of |q + dq|
whatever computes it; with |q| up to 4.5 it was 2.4e-7, which is 3e-6 of a row whose only pair gives a sum of 0.08 -- a third of the
bound spent on an addition no kernel can do better.  With 0.25 that term stays below 1e-6 of such rows, and q, mu, gmu are still five
orders of magnitude above the bound, so a kernel that dropped or doubled them fails every row.  (Changed in the cases, not in the
bound, as D_SINGLE was.)

Hub spokes.  `hubs` has 900 rows with a single pair.  Drawn up to D_SINGLE = 4 A, the worst of them stood at 5.9e-6 of the row with the
Bessel basis in float32 on the host: the phase k pi d / r_c of the 20th function is 50 rad at 4 A, half an ulp of which is 1.9e-6 rad
in any float32 arithmetic, and the error grows linearly with d.  The live spokes are therefore drawn in (0.9, ``HUB_D_NEAR`` = 2.5 A),
which is inside the D_SINGLE rule; the dead ones in (1.01, 1.12) x cutoff as elsewhere.
"""
import functools

import numpy as np
import torch

from oracle import spk_oracle as O

import cfconv_box_cases as C
from cfconv_box_cases import (CUTOFF, D_SINGLE, TILE, asymmetric, cutoff, d32, max_norm_err, reverse_edges, row_lengths, rows)  # noqa: F401

NF = 128
RT_LIVE_CAP = 256                       # spk_painn_tile.hip
ROW_WAVES = 4                           # rows per workgroup of the PaiNN row and row-tile kernels
HUB_SPOKES = (256, 257, 300, 34, 66)
HUB_LIVE = (None, 0, 1, 32, 33, "all")
RESIDUAL = 0.25
HUB_D_NEAR = 2.5                        # longest live spoke of `hubs` (module docstring)
BASES = ((16, "gaussian"), (20, "gaussian"), (23, "gaussian"), (24, "gaussian"), (31, "gaussian"), (20, "bessel"))
DECLINED = ((15, "gaussian"), (32, "gaussian"))        # no row-tile instance (kpb = n_rbf / 8 + 1 is 2 / 5); 32 keeps the fp32 forward tile kernel


# ---------------------------------------------------------------------------------------------------------
# lists
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hubs(live=None):
    """Stars whose centres have exactly 256, 257 and 300 spokes, then two of 34 and 66 (row lengths the inherited lists lack; centre first,
    then its leaves), one isolated atom before them and two after: a symmetric list of 921 atoms with rows of 0, 1, 34, 66, 256, 257
    and 300 pairs.  Every spoke is the only pair of its leaf's row:
    three quarters have d in (0.9, HUB_D_NEAR), one quarter in (1.01, 1.12) x cutoff, so each centre row holds pairs on both sides of the
    cutoff in every chunk.  live = 0, 1, 32, 33: spokes of the 256-star are pushed beyond the cutoff (or pulled inside it) until its
    centre row keeps exactly that many pairs inside the cutoff; the other stars stay as drawn.  live = "all": every spoke inside the
    cutoff.  On a skin plan the 256-row is compacted into the wave-private list (to `live` entries; with "all" the list is full to its
    last entry); the 257- and 300-rows are walked as they are, with "all" without a single dead pair."""
    rng = np.random.RandomState(500)
    a, b = [], []
    n = 1
    centres = []
    for k in HUB_SPOKES:
        centres.append(n)
        a += [n] * k; b += list(range(n + 1, n + 1 + k))
        n += k + 1
    N = n + 2
    a, b = np.array(a, dtype=np.int64), np.array(b, dtype=np.int64)
    E2 = len(a)
    far = rng.uniform(1.01 * CUTOFF, 1.12 * CUTOFF, E2)
    near = rng.uniform(0.9, HUB_D_NEAR, E2)
    d = np.where(rng.rand(E2) < 0.25, far, near)
    if live == "all":
        d = near.copy()
    elif live is not None:
        first = np.nonzero(a == centres[0])[0]
        inside = first[d[first] < CUTOFF]
        outside = first[d[first] >= CUTOFF]
        order = rng.permutation(len(inside))
        if len(inside) >= live:                           # push out all but `live`, spread over the row
            out = inside[order[:len(inside) - live]]
            d[out] = far[out]
        else:
            pull = outside[:live - len(inside)]
            d[pull] = near[pull]
    v = (C._unit(rng, E2) * d[:, None]).astype(np.float32)
    c = C._directed(N, a, b, v)
    c["info"] = {"name": "hubs_%s" % ("drawn" if live is None else live), "centres": tuple(centres), "live": live}
    return c


def walk_shape(compute_units):
    """(N, degree, conditions) of the ring list on which the XCD-contiguous atom walk of the row / row-tile kernels and the tile walk of
    the MFMA tile kernels are live with ragged ends on a device of `compute_units`: the smallest N >= 2^14 with N % 8 != 0 whose eighth
    ceil(N / 8) is no multiple of the per-XCD atom step 4 * grid / 8 (grid = 2 workgroups per compute unit, rounded up to 8), and the
    smallest even degree for which the tile count ceil(E / 32) is no multiple of 8."""
    grid_of = lambda n, cap: -(-min(cap, max(1, -(-n // ROW_WAVES))) // 8) * 8
    N = 1 << 14
    while True:
        grid = grid_of(N, 2 * compute_units)
        step = ROW_WAVES * grid // 8
        if N % 8 != 0 and (-(-N // 8)) % step != 0:
            break
        N += 1
    degree = 2
    while (-(-(N * degree) // TILE)) % 8 == 0:
        degree += 2
    tiles = -(-(N * degree) // TILE)
    tile_grid_fwd, tile_grid_bwd = grid_of(tiles, 2 * compute_units), grid_of(tiles, compute_units)
    cond = {"N": N, "degree": degree, "row_grid": grid, "atom_step": step, "atoms_per_xcd": -(-N // 8), "tiles": tiles,
            "tile_grid_fwd": tile_grid_fwd, "tile_grid_bwd": tile_grid_bwd,
            "n_at_least_2_14": N >= (1 << 14), "n_not_multiple_of_8": N % 8 != 0, "eighth_not_multiple_of_step": (-(-N // 8)) % step != 0,
            "tiles_not_multiple_of_8": tiles % 8 != 0,
            # every wave takes more than one row / every workgroup more than one tile, and the last XCD's share is short
            "row_walk_live": N >= (1 << 14) and N % 8 != 0 and (-(-N // 8)) % step != 0 and -(-N // 8) > step,
            "tile_walk_live": tiles % 8 != 0 and -(-tiles // 8) > tile_grid_fwd // 8 and -(-tiles // 8) > tile_grid_bwd // 8}
    return N, degree, cond


@functools.lru_cache(maxsize=None)
def walk(compute_units=256):
    """The ring list of walk_shape (16 385 atoms of degree 2 on 256 compute units), every pair inside the cutoff; the conditions are in
    ``info``."""
    from schnetpack_amd import synthetic as S
    N, degree, cond = walk_shape(compute_units)
    b = S.ring_graph_batch(N, degree, seed=600, dmin=0.9, dmax=D_SINGLE)
    return {"N": N, "idx_i": b["idx_i"], "idx_j": b["idx_j"], "r_ij": b["r_ij"], "info": dict(cond, name="walk")}


def live_row_counts(c):
    """Pairs of every row inside the cutoff, by the float32 test of the compaction (x^2 + y^2 + z^2 < cutoff^2)."""
    r = c["r_ij"].numpy().astype(np.float32)
    d2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]).astype(np.float32)
    return np.bincount(c["idx_i"].numpy(), weights=(d2 < np.float32(CUTOFF) * np.float32(CUTOFF)), minlength=c["N"]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------
def inputs(N, F=NF, seed=21):
    """c [N, 3F], q [N, F], mu [N, 3, F], gq [N, F], gmu [N, 3, F] (module docstring for the scales)."""
    g = torch.Generator().manual_seed(seed)
    return {"c": torch.randn(N, 3 * F, generator=g), "q": RESIDUAL * torch.randn(N, F, generator=g), "mu": RESIDUAL * torch.randn(N, 3, F, generator=g),
            "gq": torch.randn(N, F, generator=g), "gmu": RESIDUAL * torch.randn(N, 3, F, generator=g)}


@functools.lru_cache(maxsize=None)
def filter_params(n_rbf, F=NF, seed=4):
    g = torch.Generator().manual_seed(seed + 100 * n_rbf + F)
    return torch.randn(3 * F, n_rbf, generator=g) * 0.3, torch.randn(3 * F, generator=g) * 0.1


def radial_params(n_rbf, radial):
    return C.radial_params(n_rbf, radial)


@functools.lru_cache(maxsize=None)
def model_params(n_rbf, radial, n_layers, F=NF):
    """Seeded PaiNN representation (oracle names, one filter slice per interaction) with non-zero biases everywhere and the filter scaled
    as filter_params."""
    P = O.init_painn_params(F, n_layers, n_rbf, CUTOFF, seed=7, shared_filters=False, radial=radial)
    g = torch.Generator().manual_seed(8)
    P["filter_net.weight"] = torch.randn(3 * F * n_layers, n_rbf, generator=g) * 0.3
    for k in list(P):
        if k.endswith(".bias"):
            P[k] = 0.1 * torch.randn(P[k].shape, generator=g)
    return P


# ---------------------------------------------------------------------------------------------------------
# the formula, in edge blocks
# ---------------------------------------------------------------------------------------------------------
def message_ref(case, c, q, mu, wf, bf, n_rbf, radial, gq=None, gmu=None, dtype=torch.float64, block=1 << 12):
    """The PaiNN message (reference painn.py:50-66; the formula of _msg_oracle in tests/test_gpu_ops.py) over blocks of `block` edges, so
    that no [E, 3F] tensor of the whole list is held:
        W_e = (phi(d_e) wf^T + bf) f_c(d_e),  m_e = W_e o c[j],  q_out[i] = q[i] + sum_e m_q,  mu_out[i] = mu[i] + sum_e (m_R u_e + m_mu mu[j]).
    mu = None is the first interaction (mu == 0).  Returns q_out, mu_out, the sums dq, dmu and the scales scale_q, scale_mu [N]: the
    row's sum over its pairs of the absolute value of every term, maximised over channels (and x, y, z).  With gq, gmu also the
    first-order backward of <q_out, gq> + <mu_out, gmu>: gc [N, 3F], gmu_in [N, 3, F] (= gmu + sums), its sum dgmu, gr [E, 3] and
    scale_gc, scale_gmu over the by-neighbour rows."""
    N, ii, jj = case["N"], case["idx_i"], case["idx_j"]
    F = q.shape[1]
    E = len(ii)
    c, q, wf, bf = c.to(dtype), q.to(dtype), wf.to(dtype), bf.to(dtype)
    mu = torch.zeros(N, 3, F, dtype=dtype) if mu is None else mu.to(dtype)
    r_all = case["r_ij"].to(dtype)
    dq, aq = torch.zeros(N, F, dtype=dtype), torch.zeros(N, F, dtype=dtype)
    dmu, amu = torch.zeros(N, 3, F, dtype=dtype), torch.zeros(N, 3, F, dtype=dtype)
    bwd = gq is not None
    if bwd:
        gq, gmu = gq.to(dtype), gmu.to(dtype)
        gc, agc = torch.zeros(N, 3 * F, dtype=dtype), torch.zeros(N, 3 * F, dtype=dtype)
        dgmu, agmu = torch.zeros(N, 3, F, dtype=dtype), torch.zeros(N, 3, F, dtype=dtype)
        gr = torch.zeros(E, 3, dtype=dtype)
    for e0 in range(0, E, block):
        sl = slice(e0, min(e0 + block, E))
        i, j = ii[sl], jj[sl]
        r = r_all[sl].clone().requires_grad_(bwd)
        d = torch.sqrt((r * r).sum(1))
        u = r / d[:, None]
        W = O.dense(C._basis(d, n_rbf, radial, dtype), wf, bf) * O.cosine_cutoff(d, CUTOFF)[:, None]
        m = W * c[j]
        mq, mR, mm = m[:, :F], m[:, F:2 * F], m[:, 2 * F:]
        t_dir = mR[:, None, :] * u[:, :, None]
        t_mu = mm[:, None, :] * mu[j]
        dq.index_add_(0, i, mq.detach()); aq.index_add_(0, i, mq.detach().abs())
        dmu.index_add_(0, i, (t_dir + t_mu).detach()); amu.index_add_(0, i, (t_dir.abs() + t_mu.abs()).detach())
        if bwd:
            Wd = W.detach()
            gm_i = gmu[i]                                                       # [e, 3, F]
            tq = Wd[:, :F] * gq[i]
            tR = Wd[:, None, F:2 * F] * gm_i * u.detach()[:, :, None]           # three terms per channel
            tm = Wd[:, None, 2 * F:] * gm_i * mu[j]
            gc.index_add_(0, j, torch.cat([tq, tR.sum(1), tm.sum(1)], 1))
            agc.index_add_(0, j, torch.cat([tq.abs(), tR.abs().sum(1), tm.abs().sum(1)], 1))
            tg = mm.detach()[:, None, :] * gm_i
            dgmu.index_add_(0, j, tg); agmu.index_add_(0, j, tg.abs())
            gr[sl] = torch.autograd.grad((mq * gq[i]).sum() + ((t_dir + t_mu) * gm_i).sum(), r)[0]
    out = {"q_out": q + dq, "mu_out": mu + dmu, "dq": dq, "dmu": dmu, "scale_q": aq.amax(1), "scale_mu": amu.amax((1, 2))}
    if bwd:
        out.update({"gc": gc, "gmu_in": gmu + dgmu, "dgmu": dgmu, "gr": gr, "scale_gc": agc.amax(1), "scale_gmu": agmu.amax((1, 2))})
    return out


def representation_ref(case, q0, P, n_layers, n_rbf, radial, gq_out=None, gmu_out=None, want_gq0=True, dtype=torch.float64, block=1 << 12):
    """(q, mu) of `n_layers` PaiNN interaction + mixing blocks started from the scalar features q0 and mu = 0 (reference painn.py:246-256
    after the embedding; oracle.spk_oracle.painn_mixing and the context network of painn_interaction, the message through message_ref,
    one filter slice per interaction).  With gq_out / gmu_out also gr = d(<q, gq_out> + <mu, gmu_out>)/dr_ij and, if want_gq0, the
    gradient gq0 into q0 (gr does not depend on want_gq0: that is what the geometry-only launch relies on).  ``first`` is message_ref's
    result of the first interaction (forward, and backward where asked)."""
    Pd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in P.items()}
    N, F = q0.shape
    q, mu = q0.to(dtype), None
    keep = []
    first = None
    for l in range(n_layers):
        pre = "interactions.%d.interatomic_context_net." % l
        ql = q.detach().requires_grad_(gq_out is not None)
        c = O.dense(O.dense(ql, Pd[pre + "0.weight"], Pd[pre + "0.bias"], O.silu), Pd[pre + "1.weight"], Pd[pre + "1.bias"])
        wf, bf = Pd["filter_net.weight"][3 * F * l:3 * F * (l + 1)], Pd["filter_net.bias"][3 * F * l:3 * F * (l + 1)]
        m = message_ref(case, c.detach(), q, mu, wf, bf, n_rbf, radial, dtype=dtype, block=block)
        if l == 0:
            first = dict(m)
        q1 = m["q_out"].requires_grad_(gq_out is not None)
        mu1 = m["mu_out"].requires_grad_(gq_out is not None)
        q2, mu2 = O.painn_mixing(q1.unsqueeze(1), mu1, Pd, "mixing.%d." % l)
        q2 = q2.squeeze(1)
        keep.append((ql, c, q, mu, q1, mu1, q2, mu2, wf, bf))
        q, mu = q2.detach(), mu2.detach()
    out = {"q": q, "mu": mu, "first": first}
    if gq_out is not None:
        g_q, g_mu = gq_out.to(dtype), gmu_out.to(dtype)
        gr = torch.zeros(len(case["idx_i"]), 3, dtype=dtype)
        for l in reversed(range(n_layers)):
            ql, c, q_in, mu_in, q1, mu1, q2, mu2, wf, bf = keep[l]
            gq1, gmu1 = torch.autograd.grad([q2, mu2], [q1, mu1], [g_q, g_mu])
            b = message_ref(case, c.detach(), q_in, mu_in, wf, bf, n_rbf, radial, gq=gq1, gmu=gmu1, dtype=dtype, block=block)
            gr += b["gr"]
            if l == 0:
                first.update({k: b[k] for k in ("gc", "gmu_in", "dgmu", "gr", "scale_gc", "scale_gmu")})
                first["gq1"], first["gmu1"] = gq1, gmu1
                if not want_gq0:
                    break
            g_q = gq1 + torch.autograd.grad(c, ql, b["gc"])[0]
            g_mu = b["gmu_in"]
        out["gr"] = gr
        if want_gq0:
            out["gq0"] = g_q
    return out


# ---------------------------------------------------------------------------------------------------------
# error measures
# ---------------------------------------------------------------------------------------------------------
def per_row_err(got, base, ref_sum, scale):
    """The summed part of an output, per row against the row's own scale: max over the rows with scale > 0 of
    max_c |(got - base) - ref_sum| / scale[row], where `base` is the input term (q, mu, gmu_out; None for gc and for mu_out of the first
    interaction).  Rows with scale == 0 (no pair inside the cutoff) must equal `base` EXACTLY.  Returns (worst figure, its row, the
    offending rows of scale 0)."""
    N = got.shape[0]
    g = got.double().reshape(N, -1)
    b = torch.zeros_like(g) if base is None else base.double().reshape(N, -1)
    diff = ((g - b) - ref_sum.double().reshape(N, -1)).abs().amax(1)
    scale = scale.double()
    live = scale > 0
    fig = torch.where(live, diff / torch.where(live, scale, torch.ones_like(scale)), torch.zeros_like(diff))
    dead_bad = ((~live) & ((g != b).any(1))).nonzero().flatten().tolist()
    row = int(fig.argmax()) if N else 0
    return (float(fig[row]) if N else 0.0), row, dead_bad
