"""Register / scratch budget of the one-launch SchNet molecule force call (csrc/spk_schnet_mol.hip: ``k_schnet_mol_force<KPB>``), from
hipcc's kernel-resource remarks like tests/test_kernel_budget.py (no GPU needed).

The kernel is the forward and the backward launch back to back; its budget is the larger of the two halves' budgets there: at most
192 B per lane of scratch, at least two waves per SIMD, for every instance."""
import pytest

from schnetpack_amd.csrc import build as B
from test_kernel_budget import _resources

FRAGMENT = "k_schnet_mol_forceILi"
MAX_SCRATCH, MIN_OCC = 192, 2


def test_force_kernel_instances_keep_their_register_budget():
    try:
        B._hipcc()
    except Exception as exc:  # pragma: no cover
        pytest.skip("no hipcc: %s" % exc)
    rows = _resources("spk_schnet_mol.hip")
    hits = {n: r for n, r in rows.items() if FRAGMENT in n}
    assert len(hits) >= 3, "instances of k_schnet_mol_force (one to three k-blocks) not found: %s" % sorted(hits)
    assert not any("k_schnet_mol_fwdILi" in n or "k_schnet_mol_bwdILi" in n for n in hits), "the two launches' budget entries would match it"
    for name, r in sorted(hits.items()):
        print("%s: %d VGPRs, %d B/lane of scratch, %d waves/SIMD" % (name, r.get("vgpr", -1), r.get("scratch", 0), r.get("occ", 0)))
        assert r.get("scratch", 0) <= MAX_SCRATCH, "%s: %d B/lane of scratch (budget %d)" % (name, r.get("scratch", 0), MAX_SCRATCH)
        assert r.get("occ", 0) >= MIN_OCC, "%s: %d waves/SIMD (budget >= %d)" % (name, r.get("occ", 0), MIN_OCC)
