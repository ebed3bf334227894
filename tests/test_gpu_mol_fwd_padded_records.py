"""Padded forward-side records of the split molecule-resident SchNet forward (csrc/spk_schnet_mol.hip): once per group the entries
[np, 32 ntile) of the pair records become the last pair's record with f_c = 0, and the tile blocks read them at constant offsets
-- no row count, no clamp, no select.

A padded tile is compared with the SAME pairs in a full-tile layout.  The full layout appends pairs beyond the cutoff behind the P
pairs of the group (far atoms, listed in canonical order behind every pair of the base atoms) until the last tile is full; with
the molecule-resident backward switched off the forward keeps a record for each of them, with f_c = 0 exactly as a padding entry
has it.  A filter row depends on the pair's distance alone and a row of weight zero adds zero to every atom, so the filter rows
of the P pairs and the features of the base atoms must be BIT-EQUAL between the two layouts, through all interactions.  The
last pair's row is stored by its own row and by every padding row: it takes part in the same comparison, and is checked against
the float64 oracle with the project's bound 1e-5.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import mol_capacity_cases as C
import mol_fwd_operand_cases as F
from schnetpack_amd import synthetic as S
from test_gpu_mol_fwd_operands import TOL, _CForward, _filter_oracle, _model, _params, _split

pytestmark = pytest.mark.gpu
COUNTS = (1, 31, 33)            # pairs of the padded group: one tile with 1 and with 31 rows, two tiles with 32 + 1
N_FAR = 8                       # far atoms of the full layout, 6 A apart on a line 20 A from the base atoms


def _base(P):
    """(Z, R, pi, pj): two atoms with their one pair, or the 12-atom cluster of the cases with the first P of its 66 pairs in
    canonical order (every such pair has i <= 10)."""
    if P == 1:
        return [8, 1], np.array([[0.0, 0.0, 0.0], [0.96, 0.1, -0.2]]), np.array([0]), np.array([1])
    Z, R = C.cluster(12, 930)
    pi, pj = C._all_pairs(R, F.CUTOFF)
    order = np.lexsort((pj, pi))[:P]
    return list(Z), np.asarray(R, dtype=np.float64), pi[order], pj[order]


def _padded(P):
    Z, R, pi, pj = _base(P)
    return C._system(Z, R, C._directed(pi, pj))


def _full(P):
    """The base atoms and their P pairs, then N_FAR atoms whose pairs -- with the LAST base atom and among themselves, every one
    longer than 6 A -- fill the last tile: the canonical order puts them behind the P pairs."""
    Z, R, pi, pj = _base(P)
    nb, n_extra = len(Z), -P % 32
    far = np.array([[20.0 + 6.0 * k, 0.3 * k, 0.0] for k in range(N_FAR)])
    ei = [nb - 1] * N_FAR + [nb + a for a in range(N_FAR) for _ in range(a + 1, N_FAR)]
    ej = [nb + k for k in range(N_FAR)] + [nb + b for a in range(N_FAR) for b in range(a + 1, N_FAR)]
    assert n_extra <= len(ei) and (pi.max() < nb - 1 or P == 1)
    ei, ej = np.array(ei[:n_extra]), np.array(ej[:n_extra])
    Rf = np.concatenate([R, far])
    assert np.linalg.norm(Rf[ei] - Rf[ej], axis=1).min() > F.CUTOFF + 1.0
    return C._system(list(Z) + [6] * N_FAR, Rf, C._directed(np.concatenate([pi, ei]), np.concatenate([pj, ej])))


@pytest.mark.parametrize("n_rbf", [8, 16, 20, 32])
def test_padded_tile_equals_the_full_tile_layout(dev_no_mol_bwd, n_rbf):
    dev = dev_no_mol_bwd
    sep = C.loop_system("cap384")                      # 32 atoms: nothing merges across it
    systems = []
    for P in COUNTS:
        systems += [_padded(P), sep, _full(P), sep]
    b = S.collate(systems)
    rep, _ = _params(n_rbf, "gaussian", biased=True)
    with _split(True):
        fwd = _CForward(_model(n_rbf, "gaussian", biased=True), b, dev)
        x, saved, tags = fwd()
    assert "schnet_mol_fwd" in tags, tags
    atoms, pairs = np.diff(fwd.grp_atom0).tolist(), np.diff(fwd.grp_pair0).tolist()
    assert pairs[0::4] == list(COUNTS) and pairs[2::4] == [P + (-P % 32) for P in COUNTS], pairs
    assert atoms[0::4] == [2, 12, 12] and atoms[2::4] == [2 + N_FAR, 12 + N_FAR, 12 + N_FAR], atoms
    rows = fwd.filter_rows(saved)
    e = fwd.pair_edges()
    r32 = fwd.r_ij.cpu()[e].double()
    d = torch.sqrt((r32 * r32).sum(1))
    ref = _filter_oracle(rep, d)
    scale = ref[:, d < F.CUTOFF].abs().amax(dim=(1, 2))
    for k, P in enumerate(COUNTS):
        qa, qb = int(fwd.grp_pair0[4 * k]), int(fwd.grp_pair0[4 * k + 2])
        aa, ab, na = int(fwd.grp_atom0[4 * k]), int(fwd.grp_atom0[4 * k + 2]), atoms[4 * k]
        assert torch.equal(d[qa:qa + P], d[qb:qb + P]) and bool((d[qb + P:qb + P + (-P % 32)] > F.CUTOFF).all())
        same_rows = torch.equal(rows[:, qa:qa + P], rows[:, qb:qb + P])
        same_x = torch.equal(x[aa:aa + na], x[ab:ab + na])
        last = float(((rows[:, qa + P - 1].double() - ref[:, qa + P - 1]).abs().amax(dim=1) / scale).max())
        print("n_rbf=%d, %d pairs padded against %d records: filter rows bit-equal %s, features bit-equal %s, last pair's row against "
              "float64 %.3e (bound %.1e)" % (n_rbf, P, P + (-P % 32), same_rows, same_x, last, TOL))
        assert torch.isfinite(rows[:, qa:qa + P]).all() and torch.isfinite(x[aa:aa + na]).all()
        assert same_rows, (P, (rows[:, qa:qa + P] != rows[:, qb:qb + P]).any(dim=(0, 2)).nonzero().flatten().tolist())
        assert same_x, (P, (x[aa:aa + na] != x[ab:ab + na]).any(dim=1).nonzero().flatten().tolist())
        assert last < TOL


@pytest.fixture
def dev_no_mol_bwd(monkeypatch):
    """cuda:0 with the molecule-resident backward switched off: the forward then keeps the pairs beyond the cutoff as records."""
    assert torch.cuda.is_available()
    monkeypatch.setenv("SPK_NO_MOL_BWD", "1")
    return torch.device("cuda:0")
