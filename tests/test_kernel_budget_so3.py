"""Register / scratch budget of the SO(3) kernels (csrc/spk_so3.hip), from hipcc's kernel-resource remarks, by the method of
tests/test_kernel_budget.py (cross-compiles: no GPU needed).

The convolution and product kernels keep the Clebsch-Gordan operands of a lane in registers (3 S + lmax + 1 values, S = (lmax + 1)^2; the product
backward 5 S) and run the contraction as straight-line code from the compiled-in table: scratch would put memory traffic into that code, and a single
wave per SIMD could not hide the latency of the feature-row loads.  Budget: no scratch and at least 2 waves per SIMD for every instance, the floors
of tests/test_kernel_budget.py (compile remarks: profiles/so3net.md; lmax = 3 is the tight case, 177 VGPRs in the forward convolution).  The
per-pair kernels 8.
"""
import pytest

from schnetpack_amd.csrc import build as B
from test_kernel_budget import _resources

# mangled-name fragment -> (max scratch bytes per lane, min waves per SIMD, number of instances)
BUDGET = {"k_so3_conv": (0, 2, 6), "k_so3_edgeILi": (0, 2, 3), "k_so3_prod_fwd": (0, 2, 3), "k_so3_prod_bwd": (0, 2, 3), "k_so3_edge_fin": (0, 8, 1),
          "k_rsh_fwd": (0, 8, 3), "k_rsh_bwd": (0, 8, 3)}


def test_so3_kernels_have_no_scratch_and_keep_their_occupancy():
    try:
        B._hipcc()
    except Exception as exc:  # pragma: no cover
        pytest.skip("no hipcc: %s" % exc)
    assert "spk_so3.hip" in B.SOURCES
    rows = _resources("spk_so3.hip")
    assert rows, "hipcc printed no kernel-resource remarks for spk_so3.hip"
    assert len(rows) == sum(n for _, _, n in BUDGET.values()), sorted(rows)      # every kernel of the file is budgeted below
    for frag, (max_scratch, min_occ, count) in BUDGET.items():
        hits = {n: r for n, r in rows.items() if frag in n}
        assert len(hits) == count, "%d instances of %s in spk_so3.hip, expected %d (renamed? update BUDGET)" % (len(hits), frag, count)
        for name, r in sorted(hits.items()):
            print("%s: scratch %d B/lane, %d waves/SIMD, %d VGPR" % (name, r.get("scratch", 0), r.get("occ", 0), r.get("vgpr", 0)))
            assert r.get("scratch", 0) <= max_scratch, "%s: %d B/lane of scratch (budget %d)" % (name, r.get("scratch", 0), max_scratch)
            assert r.get("occ", 0) >= min_occ, "%s: %d waves/SIMD (budget >= %d)" % (name, r.get("occ", 0), min_occ)
