"""Seeded groups on the pair-tile edges of the molecule-resident SchNet forward (csrc/spk_schnet_mol.hip): a group's pairs are worked
through in tiles of 32 rows; the last tile of a group is padded, and the forward fills the padding rows of its operands from the
tile's last pair.  Shared by tests/test_mol_fwd_operand_cases.py (CPU: every case has the counts its name says, and the float32
oracle is well inside the bound on them) and tests/test_gpu_mol_fwd_operands.py.  A plain module built on the blocks of
tests/mol_capacity_cases.py: numpy only, no fixtures, every random draw seeded.

A *case* is one system that forms a group of its own in the plan; its name carries the pairs the group lists and, for the lists with
a skin, the pairs inside the 5 A cutoff.  ``batch(1)`` is every case once (``CYCLE``), each between neighbours it cannot merge with (a group holds
at most 32 atoms: a single atom stands between 32-atom clusters, the 2-atom systems between 31-atom ones, the 12-atom clusters
between aspirins); ``batch(loop_cycles())`` repeats the cycle until a launch grid of one workgroup per compute unit visits at least three groups
per workgroup, unlike ones because the cycle length and the grid size have no common period.
"""
import functools

import numpy as np

import mol_capacity_cases as C
from schnetpack_amd import synthetic as S

CUTOFF, SKIN, TILE = C.CUTOFF, C.SKIN, C.TILE

# name -> (listed pairs of the group, pairs inside the cutoff, atoms)
CASES = {
    "pairs1": (1, 1, 2),                 # one tile with ONE valid row
    "pairs31": (31, 31, 12),             # one padding row
    "pairs32": (32, 32, 12),             # exactly full
    "pairs33": (33, 33, 12),             # a second tile that holds a single pair
    "pairs63": (63, 63, 12),
    "pairs64": (64, 64, 12),
    "pairs65": (65, 65, 12),
    "far1_inside0": (1, 0, 2),           # pairs, but none inside the cutoff (6 A apart in a 7 A list)
    "atom_pairs0": (0, 0, 1),            # a single atom
    "skin190_inside162": (190, 162, 20),  # a 7 A list whose compaction leaves a ragged last tile (162 = 5 x 32 + 2)
}
SKIN_CLUSTER_SEED = 1
SEPARATORS = {"sep32": 32, "sep31": 31, "aspirin": 21}


@functools.lru_cache(maxsize=None)
def system(name):
    """The system of a case or of a separator (shared arrays: do not modify)."""
    if name in ("pairs31", "pairs32", "pairs33", "pairs63", "pairs64", "pairs65"):
        P = int(name[5:])
        return C.capped(12, P, 900 + P)
    if name == "pairs1":
        # C - O at 1.6 A.  (The forces of a two-atom system are a small difference for many separations -- the H2 dimer of the
        # capacity cases leaves the float32 oracle 3e-6 ... 3e-5 from the float64 one for some bases; this one stays below 1e-6.)
        return C._system([6, 8], np.array([[0.0, 0.0, 0.0], [1.6, 0.0, 0.0]]), (np.array([0, 1]), np.array([1, 0])), "pair")
    if name == "far1_inside0":
        return C._system([8, 1], np.array([[0.0, 0.0, 0.0], [6.0, 0.0, 0.0]]), (np.array([0, 1]), np.array([1, 0])), "far")
    if name == "atom_pairs0":
        return C.atom(902)
    if name.startswith("skin"):
        return C._full(*C.cluster(20, SKIN_CLUSTER_SEED, radius=3.3), rc=SKIN)
    if name == "sep32":
        return C.capped(32, 384, 910)
    if name == "sep31":
        return C.capped(31, 300, 911)
    if name == "aspirin":
        return C.aspirin(912)
    raise KeyError(name)


CYCLE = ("sep32", "atom_pairs0", "sep32", "sep31", "pairs1", "sep31", "far1_inside0", "sep31",
         "pairs31", "aspirin", "pairs32", "aspirin", "pairs33", "aspirin", "pairs63", "aspirin", "pairs64", "aspirin", "pairs65", "aspirin",
         "skin190_inside162", "aspirin")
DISTINCT = tuple(sorted(set(CYCLE)))


def labels(n_cycles=1):
    return CYCLE * n_cycles


def loop_cycles(compute_units=256):
    """Cycles for which every workgroup of a grid of ``compute_units`` visits at least three groups."""
    return -(-3 * compute_units // len(CYCLE))


@functools.lru_cache(maxsize=None)
def batch(n_cycles=1):
    return S.collate([system(l) for l in labels(n_cycles)])


def distinct_batch():
    """Every distinct system once: the oracle runs on this, and its rows are laid out in batch order by ``expand``."""
    return S.collate([system(l) for l in DISTINCT])


def expand(ref, n_cycles, atom_keys=("forces", "scalar_representation")):
    """Reference of ``batch(n_cycles)`` from the reference of ``distinct_batch()`` (molecules do not interact)."""
    import torch
    start = np.concatenate([[0], np.cumsum([len(system(l)["Z"]) for l in DISTINCT])])
    where = {l: k for k, l in enumerate(DISTINCT)}
    lab = labels(n_cycles)
    rows = torch.from_numpy(np.concatenate([np.arange(start[where[l]], start[where[l] + 1]) for l in lab]))
    out = {key: ref[key][rows] for key in atom_keys if key in ref}
    out["energy"] = ref["energy"][torch.tensor([where[l] for l in lab])]
    return out


def pair_distances(s):
    """float32 distances of the undirected pairs (i < j) of a system's list, in list order."""
    R = np.asarray(s["R"], dtype=np.float32)
    keep = s["idx_i"] < s["idx_j"]
    v = R[s["idx_j"][keep]] - R[s["idx_i"][keep]]
    return np.sqrt((v * v).sum(-1, dtype=np.float32))
