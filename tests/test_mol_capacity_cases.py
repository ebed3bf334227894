"""CPU checks of tests/mol_capacity_cases.py: every named case has the atom and pair counts its name promises (from
``data.host_plan``, the plan the collate workers make), and the float32 oracle stays within 3e-6 of the float64 oracle per molecule
on these inputs -- so the 1e-5 bound of tests/test_gpu_mol_capacity.py leaves the reference itself more than 3x of room."""
import numpy as np
import pytest
import torch

import mol_capacity_cases as C
from oracle import spk_oracle as O
from schnetpack_amd import synthetic as S

ORACLE_F32_BOUND = 3e-6


@pytest.mark.parametrize("name", C.ELIGIBLE_CASES)
def test_case_is_what_its_name_says(name):
    b = C.batch(name)
    p = C.plan(b)
    meta = p["meta"]
    atoms, pairs, groups = C.EXPECTED[name]
    assert meta[0] == 1 and meta[1] == 1, meta                     # sorted, symmetric
    assert meta[4] == atoms, meta                                  # max_group_atoms
    if pairs is not None:
        assert meta[5] == pairs, meta                              # max_group_pairs
    assert meta[3] == len(groups)
    assert tuple(np.diff(p["grp_atom0"]).tolist()) == groups
    assert C.min_cluster_distance(name) >= 1.0


def test_capacity_constants_match_the_plan_code():
    from schnetpack_amd import data as D
    assert C.MAX_ATOMS == D.MAX_GROUP_ATOMS == 32 and C.MAX_PAIRS == 384 and C.MAX_PAIRS % C.TILE == 0


@pytest.mark.parametrize("name,pairs,tiles,tail", [("full28", 378, 12, 26), ("cap384", 384, 12, 0), ("cap383", 383, 12, 31), ("cap353", 353, 12, 1),
                                                    ("cap352", 352, 11, 0), ("sparse32", 33, 2, 1), ("over385", 385, 13, 1)])
def test_edge_groups_have_the_pair_tiles_of_their_name(name, pairs, tiles, tail):
    p = C.plan(C.batch(name))
    atoms, npair = np.diff(p["grp_atom0"]), np.diff(p["grp_pair0"])
    edge = [g for g in range(len(atoms)) if atoms[g] == (28 if name == "full28" else 32)]
    assert len(edge) == (1 if name == "over385" else 3)
    if name != "over385":
        assert edge[0] == 0 and edge[-1] == len(atoms) - 1 and 0 < edge[1] < len(atoms) - 1         # first, in the middle, last
    for g in edge:
        assert npair[g] == pairs and (npair[g] + 31) // 32 == tiles and npair[g] % 32 == tail


def test_sparse32_has_atoms_without_pairs_and_occupies_the_last_rows():
    b = C.batch("sparse32")
    p = C.plan(b)
    deg = np.diff(p["rowptr"])
    lone_last = 0
    for g in (0, 2, 4):
        a0, a1 = p["grp_atom0"][g], p["grp_atom0"][g + 1]
        assert a1 - a0 == 32
        assert (deg[a0:a1] == 0).sum() >= 1                       # an atom with no pair inside a group with pairs
        assert (deg[a0 + 28:a1] > 0).any()                        # rows 28 .. 31 carry pairs
        lone_last += int(deg[a1 - 1] == 0)
    assert lone_last >= 1                                         # ... and once row 31 itself is an atom without pairs


def test_merge32_and_nomerge33_group_boundaries():
    p = C.plan(C.batch("merge32"))
    assert p["grp_atom0"].tolist() == [0, 32, 53, 85, 115, 147]    # 3 x 9 + 5 x 1 | 21 | 31 + 1 | 9 + 21 | 31 + 1
    p = C.plan(C.batch("nomerge33"))
    assert p["grp_atom0"].tolist() == [0, 21, 33, 61, 88, 115]     # 21 | 12 (21 + 12 = 33) | 28 | 3 x 9 | 6 + 21 (27 + 6 = 33)


def test_over33_has_no_groups_and_over385_one_pair_too_many():
    p = C.plan(C.batch("over33"))
    assert p["meta"][3] == 0 and p["grp_atom0"].size == 0
    assert max(len(s["Z"]) for s in C.case("over33")) == 33
    p = C.plan(C.batch("over385"))
    assert p["meta"][4] == 32 and p["meta"][5] == C.MAX_PAIRS + 1


def test_skin384_share_beyond_the_cutoff():
    bs, be = C.batch("skin384"), C.batch("skin384_exact")
    assert torch.equal(bs["R"], be["R"]) and torch.equal(bs["Z"], be["Z"])
    for seed in C.SKIN_SEEDS:
        Z, R, skin, exact = C.skin_cluster(32, seed)
        assert skin[0].shape[0] == 2 * C.MAX_PAIRS
        d = np.sqrt(((R[skin[1]] - R[skin[0]]) ** 2).sum(-1))
        assert d.max() < C.SKIN
        share = float(np.mean(d >= C.CUTOFF))
        assert 0.25 <= share <= 0.60, share
        assert exact[0].shape[0] == int(round((1 - share) * 2 * C.MAX_PAIRS))
        have = set(zip(skin[0].tolist(), skin[1].tolist()))
        assert all(e in have for e in zip(exact[0].tolist(), exact[1].tolist()))


def test_loop_mixed_has_more_groups_than_compute_units():
    b = C.batch("loop_mixed")
    p = C.plan(b)
    assert p["meta"][3] >= 320 and p["meta"][4] == 32 and p["meta"][5] == C.MAX_PAIRS         # 1.25 x 256 compute units
    groups = C.loop_groups()
    assert len(groups) == p["meta"][3]
    kinds = {g[2] for g in groups}
    assert {("cap384",), ("full28",)} <= kinds and any("dimer" in k for k in kinds)
    # a large group after a small one and the reverse, at a stride of the launch grid too (workgroup w takes groups w, w + 256, ...)
    big = np.array([k in (("cap384",), ("full28",)) for _, _, k in groups])
    assert (big[:-1] & ~big[1:]).any() and (~big[:-1] & big[1:]).any()
    assert (big[:-256] & ~big[256:]).any() and (~big[:-256] & big[256:]).any()


def test_loop_mixed_groups_can_be_run_alone_as_a_first_group():
    """The bit-equality check of the GPU test runs every distinct composition of a group once as the first group of a small batch."""
    compositions = {g[2] for g in C.loop_groups() if g[2] in (("cap384",), ("full28",)) or "dimer" in g[2]}
    assert 3 <= len(compositions) <= 60
    for labels in compositions:
        systems = C.loop_group_alone(labels)
        p = C.plan(S.collate(systems))
        assert p["meta"][3] == 3 and p["grp_atom0"][1] == sum(len(s["Z"]) for s in systems[:len(labels)])


@pytest.mark.parametrize("kind", ["schnet", "painn"])
@pytest.mark.parametrize("name", C.ELIGIBLE_CASES)
def test_float32_oracle_is_within_3e_6_of_float64_per_molecule(name, kind):
    b = C.batch(name)
    rep = (O.init_schnet_params if kind == "schnet" else O.init_painn_params)(128, 3, 20, C.CUTOFF)
    head = O.init_atomwise_params(128, seed=1)
    r32 = O.energy_and_forces(kind, rep, head, b, 3, dtype=torch.float32, need_rep=True)
    r64 = O.energy_and_forces(kind, rep, head, b, 3, dtype=torch.float64, need_rep=True)
    keys = ["forces", "scalar_representation"] + (["vector_representation"] if kind == "painn" else [])
    for key in keys:
        err, mol = C.per_molecule_err(r32[key], r64[key], b["idx_m"])
        assert err < ORACLE_F32_BOUND, (key, err, mol)
    err, mol = C.energy_err(r32["energy"], r64["energy"])
    assert err < ORACLE_F32_BOUND, ("energy", err, mol)
