"""The Atomwise head kernels (csrc/spk_dense.hip: k_atomwise_fwd16, k_atomwise_fwd, k_atomwise_bwd; dispatch in spk_atomwise_fwd_f32) on
the cases of tests/atomwise_head_cases.py: atom counts on both sides of the 16-, 32- and 128-atom tile and block edges, the dispatch edge
N = 32 x compute units where the same inputs change kernels, hidden widths of one to five 32-feature tiles, n_in from 32 to the widest LDS
stage of the 16-atom kernel (512) and the first width beyond it (544), absent and unaligned biases, outputs requested singly, and
molecule ids in every order: one molecule across all workgroups, every atom its own molecule, ids that no atom carries, interleaved and
descending ids, and a molecule 128 or more ids past a workgroup's first.

Bound.  The project's 1e-5 in max|got - ref| / max|ref| against the float64 formula, no margin; the same formula in
float32 on the host stays below half of it on every case (tests/test_atomwise_head_cases.py).  Exact: molecule ids without atoms hold 0.0,
rows past N and entries past n_mol keep the NaN the buffers start with, every row up to N is written, the backward is bit-equal over two
calls.  The kernel a call runs is known from the dispatch predicate (both forward kernels share one profile tag); variant SIMPLE forces
the 32-atom kernel, which is how the same inputs are sent through both.  Every figure is printed before it is asserted; the worst per
quantity and kernel are recorded in profiles/atomwise_head_edges.md."""
import functools

import pytest
import torch

import atomwise_head_cases as A

pytestmark = pytest.mark.gpu
TOL = 1e-5
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def n_cu(dev):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture
def variant():
    """use(simple): variant SIMPLE (the 32-atom forward kernel whatever the shape) or AUTO for the calls that follow; AUTO again afterwards."""
    from schnetpack_amd import _lib
    assert _lib.get_variant() == _lib.VARIANT_AUTO
    yield lambda simple: _lib.set_variant(_lib.VARIANT_SIMPLE if simple else _lib.VARIANT_AUTO)
    _lib.set_variant(_lib.VARIANT_AUTO)


@functools.lru_cache(maxsize=8)
def _on_device(n_in, H, N, name):
    c = A.make_case(n_in, H, N, name)
    d = {k: c[k].float().contiguous().cuda() for k in ("x", "w1", "b1", "w2", "b2", "wE", "wA")}
    d["idx_m"] = c["idx_m"].contiguous().cuda()
    return c, d


@functools.lru_cache(maxsize=8)
def _ref(n_in, H, N, name, act, b1=True, b2=True):
    return A.head_ref(A.make_case(n_in, H, N, name), act, b1=b1, b2=b2)


def _kernel(c, n_cu, b1_aligned=True, simple=False):
    return "fwd16" if A.takes_fwd16(c["n_in"], c["H"], c["N"], n_cu, b1_aligned, simple) else "fwd32"


def _report(label, kernel, figs, bound=TOL):
    print("%-34s | %-5s | %s%s" % (label, kernel, "  ".join("%s %.3e" % kv for kv in figs.items()), "  (bound %.0e)" % bound if bound else "  (recorded)"))
    return [(label, kernel, k, v) for k, v in figs.items() if bound is not None and not v < bound]


def _call_fwd(c, d, act, want=("pre", "y_atom", "E"), b1=True, b2=True, b1_tensor=None, check=True):
    """spk_atomwise_fwd_f32 into NaN-filled buffers with one row / entry more than the call may write.  Returns ({name: tensor}, rc)."""
    from schnetpack_amd import _lib
    f, N, H = _lib.fptr, c["N"], c["H"]
    dev = d["w1"].device
    out = {"pre": torch.full((N + 1, H), NAN, device=dev) if "pre" in want else None,
           "y_atom": torch.full((N + 1,), NAN, device=dev) if "y_atom" in want else None,
           "E": torch.full((c["n_mol"] + 1,), NAN, device=dev) if "E" in want else None}
    b1t = (b1_tensor if b1_tensor is not None else d["b1"]) if b1 else None
    rc = _lib.lib().spk_atomwise_fwd_f32(f(d["x"]), f(d["w1"]), f(b1t), f(d["w2"]), f(d["b2"] if b2 else None),
                                         _lib.iptr(d["idx_m"]) if "E" in want else None, N, c["n_in"], H, A.ACT_ID[act], c["n_mol"],
                                         f(out["pre"]), f(out["y_atom"]), f(out["E"]), _lib.stream())
    if check:
        _lib.check(rc)
    return {k: v.cpu() for k, v in out.items() if v is not None}, rc


def _check_fwd(label, kernel, c, out, ref):
    """Everything up to N / n_mol written and within the bound, nothing past it touched, ids without atoms exactly 0."""
    N, n_mol = c["N"], c["n_mol"]
    figs = {}
    for q in ("pre", "y_atom"):
        if q in out:
            got = out[q]
            assert torch.isfinite(got[:N]).all(), (label, kernel, q, "rows not written", (~torch.isfinite(got[:N].reshape(N, -1))).any(1).nonzero().flatten()[:8].tolist())
            assert torch.isnan(got[N:]).all(), (label, kernel, q, "written past N")
            figs[q] = A.rel(got[:N], ref[q])
    if "E" in out:
        got = out["E"]
        assert torch.isfinite(got[:n_mol]).all(), (label, kernel, "E", "entries not written")
        assert torch.isnan(got[n_mol:]).all(), (label, kernel, "E", "written past n_mol")
        empty = A.empty_ids(c)
        assert (got[empty] == 0).all(), (label, kernel, "E of ids without atoms", empty[(got[empty] != 0)][:8].tolist())
        figs["E"] = A.rel(got[:n_mol], ref["E"])
    return _report(label, kernel, figs)


# ---------------------------------------------------------------------------------------------------------
# a. forward through the C ABI
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", A.ACTS)
@pytest.mark.parametrize("n_in,H", A.FWD16_SHAPES + A.FWD32_SHAPES)
def test_forward_on_the_tile_edges(dev, n_cu, n_in, H, act):
    """N = 1, 15 ... 17, 31 ... 33, 127 ... 129 x one / ragged / gaps / interleaved, every shape of both kernels: pre, y_atom, E."""
    bad = []
    for N in A.TILE_NS:
        for name in A.TILE_LAYOUTS:
            c, d = _on_device(n_in, H, N, name)
            kernel = _kernel(c, n_cu)
            assert kernel == ("fwd16" if (n_in, H) in A.FWD16_SHAPES else "fwd32")
            out, _ = _call_fwd(c, d, act)
            bad += _check_fwd("%s %s" % (c["label"], act), kernel, c, out, _ref(n_in, H, N, name, act))
    assert not bad, bad


@pytest.mark.parametrize("act", A.ACTS)
@pytest.mark.parametrize("side", [0, 1])
def test_forward_on_the_dispatch_edge(dev, n_cu, side, act):
    """N = 32 x compute units (the last count of the 16-atom kernel: one tile per workgroup, twice the compute units) and one atom more (the
    32-atom kernel), one molecule over every workgroup, every atom its own, interleaved ids and a molecule beyond the LDS slots."""
    n_in, H = A.EDGE_SHAPE
    N = A.edge_ns(n_cu)[side]
    bad = []
    for name in A.EDGE_LAYOUTS:
        c, d = _on_device(n_in, H, N, name)
        kernel = _kernel(c, n_cu)
        assert kernel == ("fwd16", "fwd32")[side]
        out, _ = _call_fwd(c, d, act)
        bad += _check_fwd("%s %s" % (c["label"], act), kernel, c, out, _ref(n_in, H, N, name, act))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# b. the same inputs through both forward kernels
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", A.ACTS)
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("n_in,H", A.FWD16_SHAPES)
def test_both_forward_kernels_on_every_layout(dev, n_cu, variant, n_in, H, which, act):
    """N = 17, 129 and 32 x compute units, all seven layouts: once as dispatched (16-atom kernel), once with variant SIMPLE (32-atom kernel).  Both
    against float64 in pre, y_atom and E, and pre / y_atom against each other.  idx_m in any order is the operator's contract (the
    reference's scatter_add): a kernel that loses updates when two segments of a tile carry one molecule fails `interleaved` here."""
    N = A.both_kernel_ns(n_cu)[which]
    bad = []
    for name in A.LAYOUTS:
        c, d = _on_device(n_in, H, N, name)
        ref = _ref(n_in, H, N, name, act)
        label = "%s %s" % (c["label"], act)
        outs = {}
        for simple in (False, True):
            kernel = _kernel(c, n_cu, simple=simple)
            assert kernel == ("fwd32" if simple else "fwd16")
            variant(simple)
            outs[kernel], _ = _call_fwd(c, d, act)
            bad += _check_fwd(label, kernel, c, outs[kernel], ref)
        variant(False)
        bad += _report(label, "16/32", {q: A.rel(outs["fwd16"][q][:N], outs["fwd32"][q][:N]) for q in ("pre", "y_atom")})
        _report(label, "16/32", {"E": A.rel(outs["fwd16"]["E"][:c["n_mol"]], outs["fwd32"]["E"][:c["n_mol"]])}, None)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# c. optional arguments
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", A.ACTS)
@pytest.mark.parametrize("N", [17, 129])
@pytest.mark.parametrize("n_in,H", [(128, 64), (64, 32), (128, 96)])
def test_forward_without_biases_and_with_an_unaligned_b1(dev, n_cu, n_in, H, N, act):
    """b1 = None, b2 = None, both; and b1 as the view flat[1 : 1 + H] of an aligned buffer (a parameter inside a flat buffer): 4 bytes past a
    16-byte boundary, which by the predicate leaves the 16-atom kernel and must give the same numbers."""
    c, d = _on_device(n_in, H, N, "gaps")
    label = "%s %s" % (c["label"], act)
    bad = []
    for b1, b2 in ((False, True), (True, False), (False, False)):
        out, _ = _call_fwd(c, d, act, b1=b1, b2=b2)
        bad += _check_fwd("%s%s%s" % (label, "" if b1 else " -b1", "" if b2 else " -b2"), _kernel(c, n_cu), c, out, _ref(n_in, H, N, "gaps", act, b1, b2))
    flat = torch.zeros(H + 8, device=dev)
    view = flat[1:1 + H]
    view.copy_(d["b1"])
    assert flat.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    aligned, _ = _call_fwd(c, d, act)
    shifted, _ = _call_fwd(c, d, act, b1_tensor=view)
    kernel = _kernel(c, n_cu, b1_aligned=False)
    assert kernel == "fwd32"
    bad += _check_fwd(label + " b1+4", kernel, c, shifted, _ref(n_in, H, N, "gaps", act))
    bad += _report(label + " b1+4 vs aligned", kernel, {q: A.rel(shifted[q][:len(aligned[q]) - 1], aligned[q][:-1]) for q in ("pre", "y_atom", "E")})
    assert torch.equal(flat[:1].cpu(), torch.zeros(1)) and torch.equal(flat[1 + H:].cpu(), torch.zeros(7))
    assert not bad, bad


@pytest.mark.parametrize("act", A.ACTS)
@pytest.mark.parametrize("n_in,H,N", [(128, 64, 33), (128, 64, 129), (128, 96, 33), (128, 96, 129)])
def test_forward_outputs_requested_singly(dev, n_cu, n_in, H, N, act):
    """y_atom alone (E and idx_m null), E alone (y_atom null), both without pre, and pre + y_atom without E: each equals the full call."""
    bad = []
    for name in ("ragged", "interleaved"):
        c, d = _on_device(n_in, H, N, name)
        ref, kernel = _ref(n_in, H, N, name, act), _kernel(c, n_cu)
        full, _ = _call_fwd(c, d, act)
        for want in (("y_atom",), ("E",), ("y_atom", "E"), ("pre", "y_atom"), ("pre", "E")):
            out, _ = _call_fwd(c, d, act, want=want)
            assert set(out) == set(want)
            bad += _check_fwd("%s %s only %s" % (c["label"], act, "+".join(want)), kernel, c, out, ref)
            for q in want:
                if q != "E":                                   # E is summed with float atomics: its order may differ between calls
                    assert torch.equal(out[q][:N], full[q][:N]), (c["label"], want, q)
    assert not bad, bad


def test_forward_of_no_atoms_zeroes_the_energies(dev):
    from schnetpack_amd import _lib
    f = _lib.fptr
    c, d = _on_device(128, 64, 17, "one")
    E = torch.full((4,), NAN, device=dev)
    x0 = torch.empty(0, 128, device=dev)
    idx0 = torch.empty(0, dtype=torch.int64, device=dev)
    y0 = torch.full((1,), NAN, device=dev)
    rc = _lib.lib().spk_atomwise_fwd_f32(f(x0), f(d["w1"]), f(d["b1"]), f(d["w2"]), f(d["b2"]), _lib.iptr(d["idx_m"]), 0, 128, 64, A.ACT_ID["silu"], 3,
                                         None, f(y0), f(E), _lib.stream())
    assert rc == 0 and idx0.numel() == 0
    E, y0 = E.cpu(), y0.cpu()
    assert (E[:3] == 0).all() and torch.isnan(E[3]) and torch.isnan(y0).all()


def test_forward_refuses_what_it_does_not_cover(dev):
    """n_in = 48, n_hidden = 48, act = 0, E without idx_m, no output requested, a w2 that is not 16-byte aligned: a non-zero return code, no
    launch (by the launch profile) and untouched outputs."""
    from schnetpack_amd import _lib
    f, L = _lib.fptr, _lib.lib()
    N, n_mol = 33, 3
    idx = _lib.iptr((torch.arange(N) % 3).to(dev))
    silu = A.ACT_ID["silu"]
    T = lambda *s: torch.randn(*s, device=dev)
    x, w1, b1, w2, b2 = T(N, 64), T(32, 64), T(32), T(32), T(1)
    x48, w148, w1h48, b48, w248 = T(N, 48), T(32, 48), T(48, 64), T(48), T(48)
    w2off = torch.zeros(40, device=dev)[1:33]
    assert w2off.data_ptr() % 16 == 4
    pre, pre48, y, E = (torch.full(s, NAN, device=dev) for s in ((N, 32), (N, 48), (N,), (n_mol,)))
    s = _lib.stream()
    calls = {"n_in = 48": lambda: L.spk_atomwise_fwd_f32(f(x48), f(w148), f(b1), f(w2), f(b2), idx, N, 48, 32, silu, n_mol, f(pre), f(y), f(E), s),
             "n_hidden = 48": lambda: L.spk_atomwise_fwd_f32(f(x), f(w1h48), f(b48), f(w248), f(b2), idx, N, 64, 48, silu, n_mol, f(pre48), f(y), f(E), s),
             "act = 0": lambda: L.spk_atomwise_fwd_f32(f(x), f(w1), f(b1), f(w2), f(b2), idx, N, 64, 32, 0, n_mol, f(pre), f(y), f(E), s),
             "E without idx_m": lambda: L.spk_atomwise_fwd_f32(f(x), f(w1), f(b1), f(w2), f(b2), None, N, 64, 32, silu, n_mol, f(pre), f(y), f(E), s),
             "no output": lambda: L.spk_atomwise_fwd_f32(f(x), f(w1), f(b1), f(w2), f(b2), None, N, 64, 32, silu, n_mol, f(pre), None, None, s),
             "w2 + 4 bytes": lambda: L.spk_atomwise_fwd_f32(f(x), f(w1), f(b1), f(w2off), f(b2), None, N, 64, 32, silu, n_mol, f(pre), f(y), None, s)}
    reasons = {"n_in = 48": "not supported", "n_hidden = 48": "not supported", "act = 0": "not supported", "E without idx_m": "go together",
               "no output": "no output requested", "w2 + 4 bytes": "alignment"}
    _lib.profile_enable(True)
    _lib.profile_report()
    try:
        for what, call in calls.items():
            rc = call()
            msg = L.spk_last_error().decode()
            print("%-16s rc %d: %s" % (what, rc, msg))
            assert rc != 0 and reasons[what] in msg, (what, rc, msg)       # refused, and for the reason the case is about
        torch.cuda.synchronize()
        rep = _lib.profile_report()
    finally:
        _lib.profile_enable(False)
    assert not any("atomwise" in t for t in rep), rep
    for t in (pre, pre48, y, E):
        assert torch.isnan(t).all()
    # the same pointers in a call that is covered: the profile sees it, so the check above can fail
    _lib.profile_enable(True)
    try:
        assert L.spk_atomwise_fwd_f32(f(x), f(w1), f(b1), f(w2), f(b2), idx, N, 64, 32, silu, n_mol, f(pre), f(y), f(E), s) == 0
        torch.cuda.synchronize()
        rep = _lib.profile_report()
    finally:
        _lib.profile_enable(False)
    assert rep["atomwise_fwd"][0] == 1 and torch.isfinite(pre).all() and torch.isfinite(E).all()


# ---------------------------------------------------------------------------------------------------------
# d. backward
# ---------------------------------------------------------------------------------------------------------
def _call_bwd(c, d, act, pre, mode, with_idx=True):
    from schnetpack_amd import _lib
    f = _lib.fptr
    gx = torch.full((c["N"] + 1, c["n_in"]), NAN, device=pre.device)
    gE = d["wE"] if mode in ("gE", "both") else None
    gy = d["wA"] if mode in ("gy", "both") else None
    _lib.check(_lib.lib().spk_atomwise_bwd_f32(f(gE), f(gy), f(pre), f(d["w1"]), f(d["w2"]), _lib.iptr(d["idx_m"]) if with_idx else None, c["N"], c["n_in"], c["H"],
                                               A.ACT_ID[act], c["n_mol"], f(gx), _lib.stream()))
    return gx


@pytest.mark.parametrize("act", A.ACTS)
@pytest.mark.parametrize("n_in,H", A.BWD_SHAPES)
def test_backward_on_the_tile_edges(dev, n_in, H, act):
    """N = 1, 31 ... 33, 129 x ragged / gaps / interleaved, from the pre the forward saved, with gE only, gy_atom only (with and without idx_m) and
    both: gx against float64, bit-equal over two calls, the row after N untouched.  H = 160 walks the hidden width in three chunks of 8 k-groups."""
    bad = []
    for N in A.BWD_NS:
        for name in A.BWD_LAYOUTS:
            c, d = _on_device(n_in, H, N, name)
            pre = torch.empty(N, H, device=dev)
            from schnetpack_amd import _lib
            _lib.check(_lib.lib().spk_atomwise_fwd_f32(_lib.fptr(d["x"]), _lib.fptr(d["w1"]), _lib.fptr(d["b1"]), _lib.fptr(d["w2"]), _lib.fptr(d["b2"]), None, N, n_in, H,
                                                       A.ACT_ID[act], 0, _lib.fptr(pre), _lib.fptr(torch.empty(N, device=dev)), None, _lib.stream()))
            for mode in A.BWD_MODES:
                ref = A.head_ref(c, act, use_gE=mode != "gy", use_gy=mode != "gE")["gx"]
                gx, again = _call_bwd(c, d, act, pre, mode).cpu(), _call_bwd(c, d, act, pre, mode).cpu()
                label = "%s %s %s" % (c["label"], act, mode)
                assert torch.isfinite(gx[:N]).all(), (label, "rows not written")
                assert torch.isnan(gx[N]).all(), (label, "written past N")
                assert torch.equal(gx[:N], again[:N]), (label, "not bit-reproducible")
                if mode == "gy":
                    assert torch.equal(gx[:N], _call_bwd(c, d, act, pre, mode, with_idx=False).cpu()[:N]), (label, "idx_m changes a call without gE")
                bad += _report(label, "bwd", {"gx": A.rel(gx[:N], ref)})
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# e. operators and module
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", A.ACTS)
@pytest.mark.parametrize("name", ["interleaved", "gaps"])
@pytest.mark.parametrize("side", ["33", "edge + 1"])
def test_operators(dev, n_cu, side, name, act):
    """torch.ops.spk_hip.atomwise_forward / atomwise_backward and atomwise with autograd at (128, 64), N = 33 (16-atom kernel) and
    32 x compute units + 1 (32-atom kernel)."""
    from schnetpack_amd import torchops  # noqa: F401
    n_in, H = A.EDGE_SHAPE
    N = 33 if side == "33" else A.edge_ns(n_cu)[1]
    c, d = _on_device(n_in, H, N, name)
    kernel, label = _kernel(c, n_cu), "%s %s" % (c["label"], act)
    ref, aid, n_mol = _ref(n_in, H, N, name, act), A.ACT_ID[act], c["n_mol"]
    both = A.head_ref(c, act)["gx"]
    ops = torch.ops.spk_hip
    E, y, pre = ops.atomwise_forward(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], d["idx_m"], n_mol, aid)
    assert E.shape == (n_mol,) and y.shape == (N, 1) and pre.shape == (N, H)
    assert (E.cpu()[A.empty_ids(c)] == 0).all()
    bad = _report(label + " atomwise_forward", kernel, {"pre": A.rel(pre.cpu(), ref["pre"]), "y_atom": A.rel(y.cpu()[:, 0], ref["y_atom"]), "E": A.rel(E.cpu(), ref["E"])})
    figs = {}
    for mode, gE, gy in (("both", d["wE"], d["wA"][:, None]), ("gE", d["wE"], None), ("gy", None, d["wA"])):
        gx = ops.atomwise_backward(gE, gy, pre, d["w1"], d["w2"], d["idx_m"], n_mol, aid)
        assert gx.shape == (N, n_in)
        figs["gx " + mode] = A.rel(gx.cpu(), A.head_ref(c, act, use_gE=mode != "gy", use_gy=mode != "gE")["gx"])
    bad += _report(label + " atomwise_backward", "bwd", figs)
    zero = ops.atomwise_backward(None, None, pre, d["w1"], d["w2"], d["idx_m"], n_mol, aid)
    assert zero.shape == (N, n_in) and (zero == 0).all()
    x = d["x"].clone().requires_grad_(True)
    E2, y2 = ops.atomwise(x, d["w1"], d["b1"], d["w2"], d["b2"], d["idx_m"], n_mol, aid)
    (gx,) = torch.autograd.grad((E2 * d["wE"]).sum() + (y2[:, 0] * d["wA"]).sum(), [x])
    bad += _report(label + " atomwise + autograd", kernel, {"y_atom": A.rel(y2.detach().cpu()[:, 0], ref["y_atom"]), "E": A.rel(E2.detach().cpu(), ref["E"]), "gx": A.rel(gx.cpu(), both)})
    x = d["x"].clone().requires_grad_(True)
    E3, _ = ops.atomwise(x, d["w1"], d["b1"], d["w2"], d["b2"], d["idx_m"], n_mol, aid)
    (gx,) = torch.autograd.grad((E3 * d["wE"]).sum(), [x])
    bad += _report(label + " atomwise + autograd, E only", kernel, {"gx": A.rel(gx.cpu(), A.head_ref(c, act, use_gy=False)["gx"])})
    assert not bad, bad


@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("N", [33, 129])
def test_module_on_interleaved_molecules(dev, n_cu, N, given):
    """atomistic.Atomwise(128, aggregation_mode="avg", per_atom_output_key=...) in eval mode (the fused kernels) against its own training-mode
    route (Dense + scatter_add) and float64, with the molecule count handed in and read from idx_m[-1]; no ATen fallback on the eval call."""
    from schnetpack_amd import atomistic, properties
    from schnetpack_amd.nn.fallback import fallback_count
    n_in, H = A.EDGE_SHAPE
    c, d = _on_device(n_in, H, N, "interleaved")
    assert int(c["idx_m"][-1]) + 1 == c["n_mol"] == 3
    ref = A.head_ref(c, "silu")
    counts = torch.bincount(c["idx_m"], minlength=3)
    head = atomistic.Atomwise(n_in, aggregation_mode="avg", output_key="energy", per_atom_output_key="e_atom")
    with torch.no_grad():
        head.outnet[0].weight.copy_(c["w1"]); head.outnet[0].bias.copy_(c["b1"])
        head.outnet[1].weight.copy_(c["w2"][None, :]); head.outnet[1].bias.copy_(c["b2"])
    head = head.to(dev)
    assert head._fused_head and head.outnet[0].out_features == H

    def run(training):
        head.train(training)
        x = d["x"].clone().requires_grad_(True)
        inp = {"scalar_representation": x, properties.idx_m: d["idx_m"], properties.n_atoms: counts.to(dev)}
        if given:
            inp["_n_molecules"] = 3
        out = head(inp)
        (gx,) = torch.autograd.grad((out["energy"] * d["wE"]).sum() + (out["e_atom"][:, 0] * d["wA"]).sum(), [x])
        return out["energy"].detach().cpu(), out["e_atom"].detach().cpu()[:, 0], gx.cpu()

    before = fallback_count()
    E, y, gx = run(False)
    assert fallback_count() == before
    Et, yt, gxt = run(True)
    s = c["wE"][c["idx_m"]] / counts.double()[c["idx_m"]] + c["wA"]
    gx_ref = (s[:, None] * c["w2"][None, :] * A.act_grad("silu", ref["pre"])) @ c["w1"]
    label = "%s silu avg%s" % (c["label"], "" if given else " n_mol from idx_m")
    bad = _report(label + " eval", _kernel(c, n_cu), {"E": A.rel(E, ref["E"] / counts.double()), "y_atom": A.rel(y, ref["y_atom"]), "gx": A.rel(gx, gx_ref)})
    bad += _report(label + " training", "aten", {"E": A.rel(Et, ref["E"] / counts.double()), "y_atom": A.rel(yt, ref["y_atom"]), "gx": A.rel(gxt, gx_ref)})
    bad += _report(label + " eval vs training", "-", {"E": A.rel(E, Et), "y_atom": A.rel(y, yt), "gx": A.rel(gx, gxt)})
    assert not bad, bad
