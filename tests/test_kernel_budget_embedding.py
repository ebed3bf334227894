"""Register / scratch / LDS budget of the electronic-embedding kernels (csrc/spk_eembed.hip), from hipcc's kernel-resource remarks, by the method of
tests/test_kernel_budget.py (cross-compiles: no GPU needed).

``k_ee_stack`` keeps its accumulators in registers across barriers and its two tiles in LDS; it is latency-bound (chains of dependent matrix
instructions behind 16-byte weight loads), so it needs a second wave per SIMD to overlap a tile's loads with another tile's chain, and scratch
would put memory traffic into that chain.  Budget: no scratch anywhere; the tile kernel at least 2 waves per SIMD at F = 64, 128 and 256 --
counting both the registers (the compile remark) and the LDS of a four-wave workgroup (``spk_eembed_lds_bytes``) against the 160 KB of a compute
unit; the two small kernels 8.
"""
import pytest

from schnetpack_amd import _lib
from schnetpack_amd.csrc import build as B
from test_kernel_budget import _resources

SRC = "spk_eembed.hip"
LDS_PER_CU = 160 * 1024
# mangled-name fragment -> (max scratch bytes per lane, min waves per SIMD from the registers)
BUDGET = {"k_ee_logit": (0, 8), "k_ee_stats": (0, 8), "k_ee_stackILi1ELi1E": (0, 2), "k_ee_stackILi1ELi2E": (0, 2), "k_ee_stackILi2ELi1E": (0, 2),
          "k_ee_stackILi2ELi2E": (0, 2)}


def test_embedding_kernels_have_no_scratch_and_keep_their_occupancy():
    try:
        B._hipcc()
    except Exception as exc:  # pragma: no cover
        pytest.skip("no hipcc: %s" % exc)
    assert SRC in B.SOURCES and "-fno-slp-vectorize" not in B.flags_for(SRC)
    rows = _resources(SRC)
    assert rows, "hipcc printed no kernel-resource remarks for %s" % SRC
    assert len(rows) == len(BUDGET), sorted(rows)                  # every kernel of the file is budgeted below
    occ = {}
    for frag, (max_scratch, min_occ) in BUDGET.items():
        hits = {n: r for n, r in rows.items() if frag in n}
        assert len(hits) == 1, "kernel %s not found in %s (renamed? update BUDGET)" % (frag, SRC)
        for name, r in hits.items():
            print("%s: scratch %d B/lane, %d waves/SIMD, %d VGPR" % (name, r.get("scratch", 0), r.get("occ", 0), r.get("vgpr", 0)))
            assert r.get("scratch", 0) <= max_scratch, "%s: %d B/lane of scratch (budget %d)" % (name, r.get("scratch", 0), max_scratch)
            assert r.get("occ", 0) >= min_occ, "%s: %d waves/SIMD (budget >= %d)" % (name, r.get("occ", 0), min_occ)
            occ[frag] = r.get("occ", 0)
    lib = _lib.lib()
    for F in (64, 128, 256):
        lds = int(lib.spk_eembed_lds_bytes(F))
        assert 0 < lds <= LDS_PER_CU
        groups = LDS_PER_CU // lds                                  # four-wave workgroups per compute unit = waves per SIMD by the LDS
        for act in (1, 2):
            waves = min(groups, occ["k_ee_stackILi%dELi%dE" % (1 if F <= 128 else 2, act)])
            print("k_ee_stack F = %d, act %d: %d B of LDS per workgroup, %d waves/SIMD" % (F, act, lds, waves))
            assert waves >= 2
    assert lib.spk_eembed_lds_bytes(48) == -1 and lib.spk_eembed_lds_bytes(288) == -1
