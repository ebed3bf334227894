"""The inputs of tests/test_gpu_mol_bwd_tasks.py are what that file says (CPU): one group of exactly 32 atoms per unit with the stated
pair count, every tile count the decomposition of the backward distinguishes, and well conditioned -- the float32 oracle lies within
3e-6 of the float64 oracle per molecule (the criterion of tests/test_mol_capacity_cases.py), so the 1e-5 bound of the device test
measures the kernels and not a force near a zero of the potential."""
import numpy as np
import pytest
import torch

import mol_capacity_cases as C
import test_gpu_mol_bwd_tasks as T
from oracle import spk_oracle as O

F32_BOUND = 3e-6


def test_units_are_single_groups_with_the_stated_pairs_and_tiles():
    b = T._distinct_batch()                                    # (_collate asserts 32 atoms and the pair count of every group)
    plan = C.plan(b)
    pairs = np.diff(plan["grp_pair0"]).tolist()
    assert pairs == list(T.CYCLE)
    assert [(p + 31) // 32 for p in pairs] == [0, 1, 1, 2, 4, 5, 5, 8, 9, 12]
    assert int(plan["meta"][4]) == C.MAX_ATOMS and int(plan["meta"][5]) == C.MAX_PAIRS
    assert len(set(T.CYCLE[k % len(T.CYCLE)] != T.CYCLE[(k + 256) % len(T.CYCLE)] for k in range(len(T.CYCLE)))) == 1


@pytest.mark.parametrize("n_rbf", [8, 16, 20])
def test_float32_oracle_is_well_inside_the_bound_on_these_inputs(n_rbf):
    b = T._distinct_batch()
    rep, head = T._params(n_rbf)
    f32 = O.energy_and_forces("schnet", rep, head, b, 3)["forces"]
    err, mol = C.per_molecule_err(f32, T._reference(n_rbf)["forces"], b["idx_m"])
    print("n_rbf=%d forces: float32 oracle vs float64 %.3e (molecule %d)" % (n_rbf, err, mol))
    assert err < F32_BOUND
    _, gx0, gR = T._rep_reference(n_rbf)
    _, gx0_32, gR_32 = T._rep_reference(n_rbf, torch.float32)
    for what, a, r in (("dL/dx0", gx0_32, gx0), ("dL/dR", gR_32, gR)):
        err, mol = C.per_molecule_err(a, r, b["idx_m"])
        print("n_rbf=%d %s: float32 oracle vs float64 %.3e (molecule %d)" % (n_rbf, what, err, mol))
        assert err < F32_BOUND


def test_reproducibility_batch_is_well_conditioned():
    b = T._collate((0, 257, 384, 257, 384, 0))
    rep, head = T._params(20)
    f64 = O.energy_and_forces("schnet", rep, head, b, 3, dtype=torch.float64)["forces"]
    f32 = O.energy_and_forces("schnet", rep, head, b, 3)["forces"]
    err, _ = C.per_molecule_err(f32, f64, b["idx_m"])
    assert err < F32_BOUND
