"""Internal interfaces of schnetpack_amd/csrc are declared once: every cross-file symbol in a header that the defining file and
every user include, shared helpers in one place, no per-thread state outside the error buffer.  Text checks, no compiler, no GPU."""
import glob
import os
import re

from conftest import ROOT
from schnetpack_amd.csrc import build as B

CSRC = os.path.join(ROOT, "schnetpack_amd", "csrc")
# a function declaration at column 0 that ends in `;` (no body): return type, spk_ name, parameter list without braces
PROTO = re.compile(r"^(?!static\b|return\b|typedef\b|#)[A-Za-z_][\w \t\*:<>&\"]*?\b(spk_\w+)\s*\(([^;{}]*?)\)\s*;", re.M)


def _read(path):
    with open(path) as f:
        return f.read()


def _sources(*patterns):
    return sorted(p for pat in patterns for p in glob.glob(os.path.join(CSRC, pat)))


def test_every_header_is_a_build_dependency():
    listed = {os.path.normpath(os.path.join(CSRC, h)) for h in B.HEADERS}
    missing = [os.path.basename(h) for h in _sources("*.h") if os.path.normpath(h) not in listed]
    assert not missing, "headers not in build.HEADERS (a stale object would not be rebuilt): %s" % missing
    assert os.path.basename(B.HEADERS[-1]) == "spk_hip.h"      # build_torch_ops / build_native_example index it


def test_no_source_file_redeclares_a_header_symbol():
    declared = {}
    for h in _sources("*.h"):
        for m in PROTO.finditer(_read(h)):
            declared.setdefault(m.group(1), os.path.basename(h))
    assert {"spk_dense_chain_launch", "spk_cfconv_fwd_internal", "spk_schnet_mol_forward_ex", "spk_filter_table_lookup"} <= set(declared)
    again = []
    for src in _sources("*.hip"):
        text = _read(src)
        for m in PROTO.finditer(text):
            if m.group(1) in declared:
                again.append("%s:%d %s (declared in %s)" % (os.path.basename(src), text.count("\n", 0, m.start()) + 1, m.group(1), declared[m.group(1)]))
    assert not again, again


def test_prototype_pattern_finds_a_multi_line_declaration():
    text = "int spk_x_internal(const float* a,\n                   int n = 0);\nstatic int spk_y(int);\n  return spk_z(1);\nbool spk_w() {\n  return true;\n}\n"
    assert [m.group(1) for m in PROTO.finditer(text)] == ["spk_x_internal"]


def test_shared_definitions_occur_once():
    text = "".join(_read(p) for p in _sources("*.h", "*.hip", "*.cpp"))
    assert text.count("struct MolHeadDev") == 1
    assert text.count("define SPK_TRY") == 1
    # the matrix-tile convention of the fused kernels lives in spk_mfma_tile.h alone
    assert text.count("__builtin_amdgcn_mfma_f32_32x32x2f32") == 1
    assert text.count("(r & 3) + 8 * (r >> 2)") == 1
    assert text.count('"s_waitcnt lgkmcnt(0)\\n\\ts_barrier"') == 1
    for name in ("ml_row", "pm_row", "ee_row", "gm_row", "pair_of", "ml_ld<", "pm_ld<", "ML_MFMA", "PM_MFMA", "PM_BARRIER"):
        assert not re.search(r"\b" + re.escape(name) + (r"\b" if name[-1] != "<" else ""), text), name      # (whole names: ml_row_sums4 stays)
    home = _read(os.path.join(CSRC, "spk_mfma_tile.h"))
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in home and "(r & 3) + 8 * (r >> 2)" in home and "s_barrier" in home


def test_thread_local_state_only_in_the_error_buffer():
    users = [os.path.basename(p) for p in _sources("*.h", "*.hip", "*.cpp") if "thread_local" in _read(p)]
    assert users == ["spk_util.hip"], users
