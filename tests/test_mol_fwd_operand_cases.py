"""CPU checks of tests/mol_fwd_operand_cases.py: every case forms a group of its own with the pair counts of its name (from
``data.host_plan``), the looped batch gives every workgroup of a 256-wide grid three groups that are not all alike, and the float32
oracle stays within 3e-6 of the float64 oracle per molecule on these inputs (the margin tests/test_mol_capacity_cases.py keeps), for
every basis tests/test_gpu_mol_fwd_operands.py runs.  Also the sensitivity of what that test compares: a lost or duplicated row of a
ragged tile moves it by far more than its tolerance."""
import numpy as np
import pytest
import torch

import mol_capacity_cases as C
import mol_fwd_operand_cases as F
from oracle import spk_oracle as O

ORACLE_F32_BOUND = 3e-6
BASES = [(8, "gaussian"), (16, "gaussian"), (20, "gaussian"), (32, "gaussian"), (13, "gaussian"),
         (8, "bessel"), (16, "bessel"), (20, "bessel"), (32, "bessel"), (13, "bessel")]


def test_every_case_is_a_group_with_the_counts_of_its_name():
    b = F.batch(1)
    p = C.plan(b)
    assert p["meta"][0] == 1 and p["meta"][1] == 1 and p["meta"][3] == len(F.CYCLE), p["meta"]
    atoms, pairs = np.diff(p["grp_atom0"]), np.diff(p["grp_pair0"])
    seen = set()
    for g, label in enumerate(F.CYCLE):
        s = F.system(label)
        assert atoms[g] == len(s["Z"])                                   # no merge: the group is this system
        if label in F.SEPARATORS:
            assert atoms[g] == F.SEPARATORS[label]
            continue
        listed, inside, n_atoms = F.CASES[label]
        d = F.pair_distances(s)
        assert (atoms[g], pairs[g], d.shape[0], int((d < np.float32(F.CUTOFF)).sum())) == (n_atoms, listed, listed, inside), label
        digits = [int(t) for t in "".join(c if c.isdigit() else " " for c in label).split()]
        assert digits[0] == listed and (len(digits) == 1 or digits[1] == inside), label
        seen.add(label)
    assert seen == set(F.CASES)
    tails = {F.CASES[l][1] % F.TILE for l in F.CASES}
    assert {1, 31, 0, 2} <= tails                                        # one valid row, one padding row, full, ragged after compaction
    assert {F.CASES[l][1] for l in F.CASES} >= {1, 31, 32, 33, 63, 64, 65, 0}


def test_looped_batch_gives_every_workgroup_three_groups_that_are_not_alike():
    n = F.loop_cycles(256)
    lab = F.labels(n)
    p = C.plan(F.batch(n))
    assert p["meta"][3] == len(lab) >= 3 * 256 and p["meta"][4] == 32 and p["meta"][5] == C.MAX_PAIRS
    all_differ = 0
    for w in range(256):
        visit = lab[w::256]
        assert len(visit) >= 3 and len(set(visit[:3])) >= 2, (w, visit)
        all_differ += len(set(visit[:3])) == 3
    assert all_differ >= 128
    # every case is met as a first, a second and a third group of some workgroup
    for k in range(3):
        assert set(F.CASES) <= {lab[w + 256 * k] for w in range(256)}


@pytest.mark.parametrize("n_rbf,radial", BASES)
def test_float32_oracle_is_within_3e_6_of_float64_per_molecule(n_rbf, radial):
    b = F.distinct_batch()
    rep, head = O.init_schnet_params(128, 3, n_rbf, F.CUTOFF, radial=radial), O.init_atomwise_params(128, seed=1)
    r32 = O.energy_and_forces("schnet", rep, head, b, 3, dtype=torch.float32, need_rep=True)
    r64 = O.energy_and_forces("schnet", rep, head, b, 3, dtype=torch.float64, need_rep=True)
    for key in ("forces", "scalar_representation"):
        err, mol = C.per_molecule_err(r32[key], r64[key], b["idx_m"])
        assert err < ORACLE_F32_BOUND, (key, err, F.DISTINCT[mol])
    err, mol = C.energy_err(r32["energy"], r64["energy"])
    assert err < ORACLE_F32_BOUND, ("energy", err, F.DISTINCT[mol])


@pytest.mark.parametrize("label", ["pairs31", "pairs33", "pairs65", "skin190_inside162"])
def test_a_lost_or_duplicated_pair_of_a_ragged_tile_is_visible(label):
    """Dropping the last pair inside the cutoff from the oracle's list (the row a ragged last tile ends with), or counting it twice,
    moves the representation and the forces of that molecule by more than 100 x the 1e-5 the device test allows."""
    from schnetpack_amd import synthetic as S
    s = F.system(label)
    rep, head = O.init_schnet_params(128, 3, 20, F.CUTOFF), O.init_atomwise_params(128, seed=1)
    keep = np.nonzero((s["idx_i"] < s["idx_j"]))[0]
    R = np.asarray(s["R"], dtype=np.float32)
    d = np.sqrt(((R[s["idx_j"][keep]] - R[s["idx_i"][keep]]) ** 2).sum(-1))
    last = keep[np.nonzero(d < F.CUTOFF)[0][-1]]
    i, j = int(s["idx_i"][last]), int(s["idx_j"][last])
    both = ((s["idx_i"] == i) & (s["idx_j"] == j)) | ((s["idx_i"] == j) & (s["idx_j"] == i))
    assert both.sum() == 2
    lost = dict(s, idx_i=s["idx_i"][~both], idx_j=s["idx_j"][~both])
    twice = dict(s, idx_i=np.concatenate([s["idx_i"], s["idx_i"][both]]), idx_j=np.concatenate([s["idx_j"], s["idx_j"][both]]))
    full = O.energy_and_forces("schnet", rep, head, S.collate([s]), 3, dtype=torch.float64, need_rep=True)
    for other in (lost, twice):
        r = O.energy_and_forces("schnet", rep, head, S.collate([other]), 3, dtype=torch.float64, need_rep=True)
        for key in ("forces", "scalar_representation"):
            moved = float((r[key] - full[key]).abs().max() / full[key].abs().max())
            assert moved > 1e-3, (label, key, moved)
