"""Seeded molecule batches that sit on the capacity edges of the molecule-resident kernels (csrc/spk_schnet_mol.hip,
csrc/spk_painn_mol.hip): a group is a block-diagonal range of at most 32 atoms (``kMaxGroupAtoms`` / ``MAX_GROUP_ATOMS``) with at
most 384 undirected pairs (``ML_MAXPAIRS``; ``PM_MAXEDGES`` = 768 directed), worked through in tiles of 32 pairs.  Shared by
tests/test_mol_capacity_cases.py (CPU: every case is what its name says and leaves the float32 oracle well inside the bound) and
tests/test_gpu_mol_capacity.py (device against the float64 oracle, per molecule).  A plain module: numpy only, no fixtures, no
pytest hooks; every random draw is seeded.

A *system* is a dict ``Z, R, idx_i, idx_j`` for ``synthetic.collate``; a *case* is a list of systems.  In the named cases the edge
group appears first, in the middle and last (three different clusters), with aspirin / ethanol groups between.
"""
import functools

import numpy as np

from schnetpack_amd import synthetic as S

CUTOFF = 5.0
SKIN = 7.0
MAX_ATOMS = 32          # atoms per group
MAX_PAIRS = 384         # undirected pairs per group
TILE = 32               # pairs per tile

CAPACITY_CASES = ("full28", "cap384", "cap383", "cap353", "cap352", "sparse32", "merge32", "nomerge33")
OVER_CASES = ("over385", "over33")
SKIN_CASES = ("skin384", "skin384_exact")
ELIGIBLE_CASES = CAPACITY_CASES + OVER_CASES + SKIN_CASES          # everything but loop_mixed (the oracle check of the CPU test)
ALL_CASES = ELIGIBLE_CASES + ("loop_mixed",)


# ---------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------
def _ball(n, radius, dmin, rng):
    """n float32 points inside a ball, no two closer than dmin (random sequential addition; the test is made on the rounded point)."""
    pts = []
    while len(pts) < n:
        p = rng.uniform(-radius, radius, 3).astype(np.float32).astype(np.float64)
        if p @ p > radius * radius:
            continue
        if all(np.sqrt(((p - q) ** 2).sum()) >= dmin for q in pts):
            pts.append(p)
    return np.asarray(pts)


def cluster(n, seed, radius=2.45, dmin=1.0):
    """(Z, R): n atoms labelled from {1, 6, 8} inside a ball of 2.45 A radius, at least 1.0 A apart.  The ball's diameter is below the
    5 A model cutoff, so every pair is a neighbour pair."""
    rng = np.random.RandomState(seed)
    R = _ball(n, radius, dmin, rng)
    Z = rng.choice(np.array([1, 6, 8]), size=n)
    return [int(z) for z in Z], R


def _all_pairs(R, rc):
    """Undirected pairs (i < j) with d < rc, float32 distance test like synthetic.neighbor_pairs_open."""
    ii, jj = S.neighbor_pairs_open(np.asarray(R), rc)
    keep = ii < jj
    return ii[keep], jj[keep]


def _directed(pi, pj):
    ii, jj = np.concatenate([pi, pj]), np.concatenate([pj, pi])
    order = np.lexsort((jj, ii))
    return ii[order].astype(np.int64), jj[order].astype(np.int64)


def sub_list(R, P, seed, cutoff=CUTOFF):
    """The first P undirected pairs of a seeded permutation of all pairs with d < cutoff - 0.05, both directions, sorted by (i, j):
    a symmetric sorted list with exactly P pairs, whatever the geometry."""
    pi, pj = _all_pairs(R, cutoff - 0.05)
    assert P <= pi.shape[0], (P, pi.shape[0])
    perm = np.random.RandomState(seed).permutation(pi.shape[0])[:P]
    return _directed(pi[perm], pj[perm])


def skin_cluster(n, seed):
    """(Z, R, skin list, exact list): a cluster of 3.3 A radius (all pairs closer than 7 A), its 7 A list capped at 384 pairs and the
    same pairs restricted to d < 5 A.  The cap keeps every pair beyond 5 A and fills up with a seeded choice of the closer ones: a
    uniform choice would leave about 12 % of the list beyond the cutoff, too few for the per-call compaction to drop whole tiles."""
    Z, R = cluster(n, seed, radius=3.3)
    pi, pj = _all_pairs(R, SKIN)
    R32 = R.astype(np.float32)
    inside = np.sqrt(((R32[pj] - R32[pi]) ** 2).sum(-1, dtype=np.float32)) < np.float32(CUTOFF)
    far, near = np.nonzero(~inside)[0], np.nonzero(inside)[0]
    assert far.shape[0] < MAX_PAIRS <= pi.shape[0]
    keep = np.concatenate([far, np.random.RandomState(seed + 1).permutation(near)[:MAX_PAIRS - far.shape[0]]])
    exact = keep[far.shape[0]:]
    return Z, R, _directed(pi[keep], pj[keep]), _directed(pi[exact], pj[exact])


def _system(Z, R, lst, tag="cluster"):
    return {"Z": list(Z), "R": np.asarray(R, dtype=np.float64), "idx_i": lst[0], "idx_j": lst[1], "tag": tag}


def _full(Z, R, rc=CUTOFF, tag="cluster"):
    return _system(Z, R, S.neighbor_pairs_open(np.asarray(R), rc), tag)


def aspirin(seed, rc=CUTOFF):
    rng = np.random.RandomState(seed)
    return _full(S.ASPIRIN_Z, np.asarray(S.ASPIRIN_R) + 0.05 * rng.randn(21, 3), rc, "aspirin")


def ethanol(seed, rc=CUTOFF):
    rng = np.random.RandomState(seed)
    return _full(S.ETHANOL_Z, np.asarray(S.ETHANOL_R) + 0.05 * rng.randn(9, 3), rc, "ethanol")


def atom(seed):
    rng = np.random.RandomState(seed)
    return _system([8], rng.randn(1, 3), (np.zeros(0, np.int64), np.zeros(0, np.int64)), "atom")


def dimer(seed):
    rng = np.random.RandomState(seed)
    return _system([1, 1], np.array([[0.0, 0.0, 0.0], [0.74 + 0.05 * rng.randn(), 0.0, 0.0]]), (np.array([0, 1]), np.array([1, 0])), "dimer")


def capped(n, P, seed, list_seed=None):
    """An n-atom cluster with exactly P pairs."""
    Z, R = cluster(n, seed)
    return _system(Z, R, sub_list(R, P, seed + 7 if list_seed is None else list_seed))


def _framed(edge):
    """edge(k), k = 0, 1, 2: the edge group first, in the middle and last; aspirin + ethanol (one merged group of 30 atoms) between."""
    return [edge(0), aspirin(11), ethanol(12), edge(1), ethanol(13), aspirin(14), edge(2)]


# ---------------------------------------------------------------------------------------------------------
# named cases
# ---------------------------------------------------------------------------------------------------------
# sparse32: list seeds for which the 33 pairs keep atoms 0 ... 31 in ONE group of the plan and leave at least one atom without any
# pair (seeds 0 and 6: two and eight such atoms inside the block; seed 27: atom 31 itself has no pair and joins as a block of one)
SPARSE_LIST_SEEDS = (0, 27, 6)

# skin_cluster seeds: 25 .. 60 % of the 384 listed pairs lie beyond 5 A (asserted by the CPU test; the three seeds of 700 .. 3699
# with the most such pairs: 107, 106 and 105 of 496)
SKIN_SEEDS = (1507, 3233, 2237)

# loop_mixed: units drawn by a seeded RNG; every unit of a kind is the same instance, so the reference of a kind is computed once
LOOP_KINDS = ("cap384", "full28", "ethanol3", "dimer", "aspirin")
LOOP_UNITS = 420
LOOP_SEED = 20


@functools.lru_cache(maxsize=None)
def loop_unit(kind):
    """The systems of one unit of loop_mixed."""
    if kind == "cap384":
        return (capped(32, 384, 500),)
    if kind == "full28":
        return (_full(*cluster(28, 510)),)
    if kind == "ethanol3":
        return (ethanol(521), ethanol(522), ethanol(523))
    if kind == "dimer":
        return (dimer(530),)
    if kind == "aspirin":
        return (aspirin(540),)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def loop_order(n_units=LOOP_UNITS):
    """Kinds of the units of loop_mixed, in batch order."""
    rng = np.random.RandomState(LOOP_SEED)
    return tuple(LOOP_KINDS[k] for k in rng.randint(0, len(LOOP_KINDS), size=n_units))


def loop_system(label):
    """System of a label: the kind of a one-system unit, or "ethanol3.k" for the k-th ethanol of that unit."""
    kind, _, k = label.partition(".")
    return loop_unit(kind)[int(k or 0)]


def loop_systems(n_units=LOOP_UNITS):
    """(systems, label of every system), in batch order."""
    labels = []
    for kind in loop_order(n_units):
        n = len(loop_unit(kind))
        labels += [kind] if n == 1 else ["%s.%d" % (kind, k) for k in range(n)]
    return [loop_system(l) for l in labels], labels


@functools.lru_cache(maxsize=None)
def loop_groups(n_units=LOOP_UNITS):
    """Groups of the plan of loop_mixed: (first system, one past its last system, labels of its systems).  The greedy merge joins a
    dimer, an aspirin or an ethanol to its neighbours whenever 32 atoms allow it, so a group is not always one unit."""
    systems, labels = loop_systems(n_units)
    atom0 = plan(S.collate(systems))["grp_atom0"]
    start = np.concatenate([[0], np.cumsum([len(s["Z"]) for s in systems])])
    sys0 = np.searchsorted(start, atom0)
    assert np.array_equal(start[sys0], atom0)                      # no system is cut by a group boundary
    return tuple((int(a), int(b), tuple(labels[a:b])) for a, b in zip(sys0[:-1], sys0[1:]))


def loop_group_alone(labels):
    """The systems of one group of loop_mixed as the FIRST group of a three-group batch (a 32-atom cluster follows, so nothing
    merges into it)."""
    return [loop_system(l) for l in labels] + [loop_system("cap384"), loop_system("aspirin")]


@functools.lru_cache(maxsize=None)
def case(name):
    """Systems of a named case (tuple; the arrays are shared and must not be modified)."""
    if name == "full28":           # a genuine neighbour list: 28 atoms, all 378 pairs -- 12 tiles, the last with 26 pairs
        return tuple(_framed(lambda k: _full(*cluster(28, 100 + k))))
    if name in ("cap384", "cap383", "cap353", "cap352", "over385"):
        P = int(name[-3:])
        edge = lambda k: capped(32, P, 200 + 10 * (P % 100) + k)
        if name == "over385":       # one group over the pair capacity among ordinary ones
            return (aspirin(11), ethanol(12), edge(0), ethanol(13), aspirin(14))
        return tuple(_framed(edge))
    if name == "sparse32":         # rows 28 .. 31 occupied, atoms without any pair inside a group with pairs
        return tuple(_framed(lambda k: capped(32, 33, 300 + k, SPARSE_LIST_SEEDS[k])))
    if name == "merge32":          # merged by the plan to exactly 32 atoms: 27 + 5 x 1, and 31 + 1
        return (ethanol(21), ethanol(22), ethanol(23), atom(24), atom(25), atom(26), atom(27), atom(28),
                aspirin(11), capped(31, 300, 400), atom(29), ethanol(12), aspirin(14),
                capped(31, 384, 401), atom(30))
    if name == "nomerge33":        # 21 + 12 = 33 and 27 + 6 = 33: one atom too many to merge
        return (aspirin(11), _full(*cluster(12, 410)), _full(*cluster(28, 411)), ethanol(21), ethanol(22), ethanol(23),
                _full(*cluster(6, 412)), aspirin(14))
    if name == "over33":           # one block of 33 atoms among small molecules: no grouping at all
        return (aspirin(11), ethanol(12), capped(33, 300, 420), ethanol(13), aspirin(14))
    if name in SKIN_CASES:         # 7 A lists (the cluster's capped at 384 pairs) / the same pairs inside 5 A
        skin = name == "skin384"
        rc = SKIN if skin else CUTOFF

        def edge(k):
            Z, R, lst_skin, lst_exact = skin_cluster(32, SKIN_SEEDS[k])
            return _system(Z, R, lst_skin if skin else lst_exact)
        return (edge(0), aspirin(11, rc), ethanol(12, rc), edge(1), ethanol(13, rc), aspirin(14, rc), edge(2))
    if name == "loop_mixed":
        return tuple(loop_systems()[0])
    raise KeyError(name)


# expected plan of the eligible cases: (max_group_atoms, max_group_pairs, atoms of the groups in order or None)
_F = (21 + 9, 9 + 21)           # the two merged groups between the edge groups of _framed
EXPECTED = {
    "full28": (30, 378, (28,) + _F[:1] + (28,) + _F[1:] + (28,)),
    "cap384": (32, 384, (32, 30, 32, 30, 32)),
    "cap383": (32, 383, (32, 30, 32, 30, 32)),
    "cap353": (32, 353, (32, 30, 32, 30, 32)),
    "cap352": (32, 352, (32, 30, 32, 30, 32)),
    "sparse32": (32, 153 + 36, (32, 30, 32, 30, 32)),
    "merge32": (32, 384, (32, 21, 32, 30, 32)),
    "nomerge33": (28, 378, (21, 12, 28, 27, 27)),
    "over385": (32, 385, (30, 32, 30)),
    "over33": (0, 0, ()),
    "skin384": (32, 384, (32, 30, 32, 30, 32)),
    "skin384_exact": (32, None, (32, 30, 32, 30, 32)),
}


def batch(name):
    return S.collate(list(case(name)))


def plan(b):
    """data.host_plan of a collated batch."""
    from schnetpack_amd import data as D
    return D.host_plan(b["idx_i"].numpy(), b["idx_j"].numpy(), b["offsets"].numpy(), int(b["Z"].shape[0]))


def min_cluster_distance(name):
    """Smallest distance between two atoms of one generated cluster of a case (aspirin, ethanol and the H2 dimer have their bond
    lengths)."""
    best = np.inf
    for s in case(name):
        if s["tag"] == "cluster" and len(s["Z"]) > 1:
            r = np.asarray(s["R"], dtype=np.float32).astype(np.float64)
            d = np.sqrt(((r[:, None] - r[None]) ** 2).sum(-1))
            best = min(best, d[np.triu_indices(r.shape[0], 1)].min())
    return float(best)


# ---------------------------------------------------------------------------------------------------------
# the metric: per molecule, never normalised by the rest of the batch
# ---------------------------------------------------------------------------------------------------------
def _np(t):
    return np.asarray(t.detach().cpu().double().numpy() if hasattr(t, "detach") else t, dtype=np.float64)


def per_molecule_err(got, ref, idx_m, floor=1e-12):
    """max over the molecules of max|got - ref| / max|ref|, both maxima over the rows of ONE molecule (idx_m [N], got / ref [N, ...]).
    Molecules whose reference maximum is below ``floor`` are skipped (the vector representation of a single atom is zero).
    Returns (worst error, molecule that has it); NaN / Inf in ``got`` give inf."""
    got, ref, idx_m = _np(got), _np(ref), np.asarray(_np(idx_m), dtype=np.int64)
    assert got.shape == ref.shape and got.shape[0] == idx_m.shape[0], (got.shape, ref.shape, idx_m.shape)
    n_mol = int(idx_m.max()) + 1
    diff = np.abs(got - ref).reshape(got.shape[0], -1).max(1)
    diff = np.where(np.isfinite(diff), diff, np.inf)
    mag = np.abs(ref).reshape(ref.shape[0], -1).max(1)
    num, den = np.zeros(n_mol), np.zeros(n_mol)
    np.maximum.at(num, idx_m, diff)
    np.maximum.at(den, idx_m, mag)
    ok = den >= floor
    err = np.where(ok, num / np.where(ok, den, 1.0), 0.0)
    worst = int(np.argmax(err))
    return float(err[worst]), worst


def energy_err(got, ref):
    """max over the molecules of |E - E_ref| / |E_ref|."""
    got, ref = _np(got), _np(ref)
    assert got.shape == ref.shape
    err = np.abs(got - ref) / np.abs(ref)
    err = np.where(np.isfinite(err), err, np.inf)
    worst = int(np.argmax(err))
    return float(err[worst]), worst
