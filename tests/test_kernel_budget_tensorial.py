"""Register / scratch budget of the tensorial-head kernels (csrc/spk_tensorial.hip), from hipcc's kernel-resource remarks, by the method of
tests/test_kernel_budget.py (cross-compiles: no GPU needed).

The gated-MLP kernel keeps three 32 x 32 accumulators (one per Cartesian axis) next to its operand stream; pushed into scratch it would
re-read them around every matrix instruction.  Its workgroups are placed by their LDS (one 32-atom tile of s, v and the block-0
intermediates: 101 KB at n_in = 128, 53 KB at 64), so the waves per SIMD pinned here only have to stay at or above what that allows
(256 threads = one wave per SIMD and workgroup; 1 and 3 workgroups per CU).  Compile remarks: 3 waves/SIMD (88 VGPR + 48 AGPR) at 128,
4 at 64; the moment kernels 8.
"""
import pytest

from schnetpack_amd.csrc import build as B
from test_kernel_budget import _resources

SRC = "spk_tensorial.hip"
# mangled-name fragment -> (max scratch bytes per lane, min waves per SIMD)
BUDGET = {"k_gated_mlpILi128ELi2E": (0, 3), "k_gated_mlpILi64ELi2E": (0, 4), "k_momentILi0E": (0, 8), "k_momentILi1E": (0, 8)}


def test_tensorial_kernels_have_no_scratch_and_keep_their_occupancy():
    try:
        B._hipcc()
    except Exception as exc:  # pragma: no cover
        pytest.skip("no hipcc: %s" % exc)
    assert SRC in B.SOURCES
    rows = _resources(SRC)
    assert rows, "hipcc printed no kernel-resource remarks for %s" % SRC
    kernels = {n: r for n, r in rows.items() if "k_gated_mlp" in n or "k_moment" in n}
    assert len(kernels) == 4, sorted(rows)                  # every kernel of the file is budgeted below
    for frag, (max_scratch, min_occ) in BUDGET.items():
        hits = {n: r for n, r in kernels.items() if frag in n}
        assert len(hits) == 1, "kernel %s not found in %s (renamed? update BUDGET)" % (frag, SRC)
        for name, r in hits.items():
            print("%s: scratch %d B/lane, %d waves/SIMD, %d VGPR" % (name, r.get("scratch", 0), r.get("occ", 0), r.get("vgpr", 0)))
            assert r.get("scratch", 0) <= max_scratch, "%s: %d B/lane of scratch (budget %d)" % (name, r.get("scratch", 0), max_scratch)
            assert r.get("occ", 0) >= min_occ, "%s: %d waves/SIMD (budget >= %d)" % (name, r.get("occ", 0), min_occ)
