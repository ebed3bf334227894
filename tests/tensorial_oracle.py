"""Float64 numpy restatement of the tensorial heads (a plain module, not collected by pytest): the gated equivariant block and MLP
(nn/equivariant.py:57-71, nn/blocks.py:79-156), ``DipoleMoment`` and ``Polarizability`` (atomistic/atomwise.py:172-213, :267-293).
tests/test_tensorial_reference.py pins it to the fixture the reference's own code produced (tests/golden/tensorial_cases.npz); the device
tests feed it with what the kernels were given."""
import numpy as np

#: fixture cases (tests/make_tensorial_golden.py): tag -> (n_in, n_layers, n_hidden or 0 for the pyramidal default)
CASES = {"a": (64, 2, 0), "b": (128, 2, 0), "c": (128, 2, 0), "e": (64, 3, 48)}
#: dipole variants stored per case: name -> (correct_charges, with total_charge)
VARIANTS = {"plain": (True, False), "Q": (True, True), "nocorr": (False, False)}


def silu(x):
    return x / (1.0 + np.exp(-x))


def gated_block(s, v, w, sact):
    """One block: w = (mix_vectors.weight, scalar_net.0.weight, scalar_net.0.bias, scalar_net.1.weight, scalar_net.1.bias)."""
    wm, w1, b1, w2, b2 = [np.asarray(x, dtype=np.float64) for x in w]
    m = wm.shape[0] // 2
    vmix = v @ wm.T                                   # [N, 3, 2 m]
    V, W = vmix[..., :m], vmix[..., m:]
    Vn = np.sqrt((V * V).sum(axis=-2))                # no epsilon
    x = silu(np.concatenate([s, Vn], axis=-1) @ w1.T + b1) @ w2.T + b2
    n_sout = w2.shape[0] - m
    s_out, g = x[..., :n_sout], x[..., n_sout:]
    v_out = g[:, None, :] * W
    return (silu(s_out) if sact else s_out), v_out


def gated_mlp(s, v, weights):
    """weights: flat list, five arrays per block; every block but the last applies the scalar activation."""
    s, v = np.asarray(s, dtype=np.float64), np.asarray(v, dtype=np.float64)
    n = len(weights) // 5
    for b in range(n):
        s, v = gated_block(s, v, weights[5 * b:5 * b + 5], sact=b < n - 1)
    return s, v


def mlp(x, weights):
    """build_mlp: weights = (w, b) per layer, silu on every layer but the last."""
    x = np.asarray(x, dtype=np.float64)
    n = len(weights) // 2
    for l in range(n):
        x = x @ np.asarray(weights[2 * l], dtype=np.float64).T + np.asarray(weights[2 * l + 1], dtype=np.float64)
        if l < n - 1:
            x = silu(x)
    return x


def segment_sum(x, idx_m, n_mol):
    out = np.zeros((n_mol,) + x.shape[1:], dtype=np.float64)
    np.add.at(out, idx_m, x)
    return out


def dipole(q, d, R, idx_m, n_mol, total=None, correct=True):
    """(mu [n_mol, 3], charges [N, 1]); q [N, 1], d [N, 3] or None.  Molecules without atoms: zero."""
    q, R = np.asarray(q, dtype=np.float64).reshape(-1, 1), np.asarray(R, dtype=np.float64)
    if correct:
        sq = segment_sum(q, idx_m, n_mol)
        cnt = np.bincount(idx_m, minlength=n_mol).astype(np.float64)[:, None]
        tot = np.zeros_like(sq) if total is None else np.asarray(total, dtype=np.float64).reshape(-1, 1)
        corr = np.divide(tot - sq, cnt, out=np.zeros_like(sq), where=cnt > 0)
        q = q + corr[idx_m]
    y = R * q
    if d is not None:
        y = y + np.asarray(d, dtype=np.float64).reshape(-1, 3)
    return segment_sum(y, idx_m, n_mol), q


def polarizability(a0, d, R, idx_m, n_mol):
    a0, d, R = np.asarray(a0, dtype=np.float64).reshape(-1), np.asarray(d, dtype=np.float64).reshape(-1, 3), np.asarray(R, dtype=np.float64)
    mur = d[:, :, None] * R[:, None, :]
    alpha = a0[:, None, None] * np.eye(3)[None] + mur + mur.transpose(0, 2, 1)
    return segment_sum(alpha, idx_m, n_mol)


def case_inputs(gold, tag):
    """Every array of case ``tag`` without its prefix; ``gm`` / ``ds`` = the weight lists of the gated and of the scalar head."""
    pre = tag + "_"
    c = {k[len(pre):]: gold[k] for k in gold.files if k.startswith(pre)}
    wpre = ("b" if tag == "c" else tag) + "_"            # (case c is case b with one vector row zeroed: it reads b's weights)
    c["gm"] = [gold[wpre + "gm_w%d" % k] for k in range(5 * CASES[tag][1])]
    if wpre + "ds_w0" in gold.files:
        c["ds"] = [gold[wpre + "ds_w%d" % k] for k in range(4)]
    return c


def evaluate(c):
    """Every stored output of a case from its inputs and weights."""
    idx_m, n_mol, R = c["idx_m"], int(c["n_mol"]), c["R"]
    out = {}
    q, d = gated_mlp(c["s"], c["v"], c["gm"])
    out["gm_s"], out["gm_v"] = q, d
    for name, (correct, with_q) in VARIANTS.items():
        mu, ch = dipole(q, d[..., 0], R, idx_m, n_mol, c["total_charge"] if with_q else None, correct)
        out["mu_" + name], out["charges_" + name] = mu, ch
    out["mag_plain"] = np.sqrt((out["mu_plain"] ** 2).sum(axis=1))
    out["alpha"] = polarizability(q[:, 0], d[..., 0], R, idx_m, n_mol)
    if "ds" in c:
        qs = mlp(c["s"], c["ds"])
        out["ds_q"] = qs
        for name, (correct, with_q) in VARIANTS.items():
            mu, ch = dipole(qs, None, R, idx_m, n_mol, c["total_charge"] if with_q else None, correct)
            out["ds_mu_" + name], out["ds_charges_" + name] = mu, ch
    return out
