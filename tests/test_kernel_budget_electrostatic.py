"""Register / scratch budget of the electrostatics kernels (csrc/spk_coulomb.hip, csrc/spk_ewald.hip), from hipcc's kernel-resource remarks, by
the method of tests/test_kernel_budget.py (cross-compiles: no GPU needed).

The two N x K kernels of the reciprocal-space sum -- ``k_ewald_sfac`` (a k-vector per lane, S(k) in registers over the staged atoms) and
``k_ewald_bwd`` (a wave per atom, lanes over k) -- do a handful of LDS reads and about twenty vector instructions per (atom, k): they hide that
latency only with several waves per SIMD, and scratch would put memory traffic into the inner loop.  Budget: no scratch, at least 4 waves per
SIMD (compile remarks: 36 and 50 VGPRs, 8 waves/SIMD each); the pair kernels and the small kernels 8.
"""
import pytest

from schnetpack_amd.csrc import build as B
from test_kernel_budget import _resources

# file -> mangled-name fragment -> (max scratch bytes per lane, min waves per SIMD)
BUDGET = {"spk_ewald.hip": {"k_ewald_sfac": (0, 4), "k_ewald_bwd": (0, 4), "k_ewald_reduce": (0, 8), "k_ewald_cell": (0, 8)},
          "spk_coulomb.hip": {"k_coul_row": (0, 8), "k_coul_edgeILi0E": (0, 8), "k_coul_edgeILi1E": (0, 8), "k_coul_atom": (0, 8), "k_coul_chunk": (0, 8),
                              "k_coul_mol": (0, 8)}}


@pytest.mark.parametrize("src", sorted(BUDGET))
def test_electrostatics_kernels_have_no_scratch_and_keep_their_occupancy(src):
    try:
        B._hipcc()
    except Exception as exc:  # pragma: no cover
        pytest.skip("no hipcc: %s" % exc)
    assert src in B.SOURCES
    rows = _resources(src)
    assert rows, "hipcc printed no kernel-resource remarks for %s" % src
    assert len(rows) == len(BUDGET[src]), sorted(rows)                  # every kernel of the file is budgeted below
    for frag, (max_scratch, min_occ) in BUDGET[src].items():
        hits = {n: r for n, r in rows.items() if frag in n}
        assert len(hits) == 1, "kernel %s not found in %s (renamed? update BUDGET)" % (frag, src)
        for name, r in hits.items():
            print("%s: scratch %d B/lane, %d waves/SIMD, %d VGPR" % (name, r.get("scratch", 0), r.get("occ", 0), r.get("vgpr", 0)))
            assert r.get("scratch", 0) <= max_scratch, "%s: %d B/lane of scratch (budget %d)" % (name, r.get("scratch", 0), max_scratch)
            assert r.get("occ", 0) >= min_occ, "%s: %d waves/SIMD (budget >= %d)" % (name, r.get("occ", 0), min_occ)
