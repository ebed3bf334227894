"""Which fused chain kernel the general representation drivers reach.

The first chain of each driver writes a region of ``saved`` that depends on nothing but the input features and that chain:

* SchNet (spk_schnet_forward_f32): h_0 = saved[:N F] = in2f_0(x0), a one-layer chain;
* PaiNN (spk_painn_forward_f32): preA_0 = saved[:N F], the pre-activation of the first layer of the two-layer context chain.

The comparator is the same layer(s) through the C ABI (spk_dense_chain_f32 on spk_pack_weight_f32 images, trans = 2), which carries no
split-precision images and therefore always runs the fp32 kernels.  With 32-row tiles and the split path on, the drivers run the
split-precision chain kernel on the images of their own weight pack: the result differs from fp32 in the last bits and stays within
1e-6 of it relative to the largest entry (the bound of the split product, DESIGN.md and test_gpu_mol_dense_operands.py).  16-row tiles
have no split form.  Nothing a driver call does may reach a later call of the C ABI on the same host thread.

Inputs: a periodic water box of 192 atoms (not block-diagonal: the general drivers run, no molecule-resident launch), F = n_filters =
128, one interaction, seeded oracle parameters.
"""
import ctypes

import pytest
import torch

from chain_helpers import chain_struct, pack
from oracle import spk_oracle as O
from schnetpack_amd import synthetic as S

pytestmark = pytest.mark.gpu

F = 128
SPLIT_BOUND = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


class _switches:
    """Row-tile height of the chain kernels and the split path for the calls inside; both restored on exit."""

    def __init__(self, rows, split):
        self.rows, self.split = rows, split

    def __enter__(self):
        from schnetpack_amd import _lib
        self.before = _lib.get_split()
        _lib.lib().spk_chain_set_rows(self.rows)
        _lib.set_split(self.split)

    def __exit__(self, *exc):
        from schnetpack_amd import _lib
        _lib.lib().spk_chain_set_rows(0)
        _lib.set_split(bool(self.before))


class _Box:
    """The water box on the device with its edge plan, radial basis and the buffers both drivers need."""

    def __init__(self, dev):
        from schnetpack_amd import _lib, ops
        self._lib, self.lib, self.dev = _lib, _lib.lib(), dev
        b = S.water_box(n_side=4)
        self.Z = b["Z"]
        self.N = int(self.Z.shape[0])
        assert self.N == 192
        R = b["R"].to(dev)
        ii, jj = b["idx_i"].to(dev), b["idx_j"].to(dev)
        self.r_ij = (R[jj] - R[ii] + b["offsets"].to(dev)).float().contiguous()
        self.plan = ops.EdgePlan(ii, jj, self.N, self.r_ij)
        self.keep = []

    def D(self, t):
        t = t.float().contiguous().to(self.dev)
        self.keep.append(t)
        return t

    def radial(self, p):
        from schnetpack_amd import ops
        p0, p1 = self.D(p["radial_basis.offsets"]), self.D(p["radial_basis.widths"])
        return ops.radial_struct(self._lib.SPK_RBF_GAUSSIAN, int(p0.shape[0]), p0, p1, float(p["cutoff_fn.cutoff"]))

    def profiled(self, fn):
        """fn() with the launch profile on: a chain launch ran and no molecule-resident forward did."""
        _lib = self._lib
        _lib.profile_enable(True)
        _lib.profile_report()
        try:
            out = fn()
            torch.cuda.synchronize()
            tags = set(_lib.profile_report())
        finally:
            _lib.profile_enable(False)
        assert any(t.startswith("chain") for t in tags), tags
        assert not any(t.endswith("_mol_fwd") for t in tags), tags
        return out


class _Schnet(_Box):
    def __init__(self, dev):
        super().__init__(dev)
        _lib = self._lib
        p = O.init_schnet_params(n_interactions=1)
        pre = "interactions.0."
        t = {"in2f_w": p[pre + "in2f.weight"], "fn_w1": p[pre + "filter_network.0.weight"], "fn_b1": p[pre + "filter_network.0.bias"],
             "fn_w2": p[pre + "filter_network.1.weight"], "fn_b2": p[pre + "filter_network.1.bias"], "f2out_w1": p[pre + "f2out.0.weight"],
             "f2out_b1": p[pre + "f2out.0.bias"], "f2out_w2": p[pre + "f2out.1.weight"], "f2out_b2": p[pre + "f2out.1.bias"]}
        t.update({k + "T": t[k].t() for k in ("in2f_w", "f2out_w1", "f2out_w2")})
        self.w = {k: self.D(v) for k, v in t.items()}
        self.layers = (_lib.SchnetLayerT * 1)()
        for k, v in self.w.items():
            setattr(self.layers[0], k, v.data_ptr())
        self.m = _lib.SchnetT(F, F, 1, 1, self.layers, None)
        n_pack = int(self.lib.spk_schnet_packed_floats(ctypes.byref(self.m)))
        assert n_pack > 0
        self.wpack = torch.empty(n_pack, dtype=torch.float32, device=dev)
        _lib.check(self.lib.spk_schnet_pack_weights_f32(ctypes.byref(self.m), _lib.fptr(self.wpack), _lib.stream()))
        self.m.wpack = self.wpack.data_ptr()
        self.rb = self.radial(p)
        self.x0 = self.D(p["embedding.weight"][self.Z])
        self.n_saved = int(self.lib.spk_schnet_saved_floats_graph(ctypes.byref(self.m), self.plan.graph(), ctypes.byref(self.rb)))
        self.scratch = torch.empty(int(self.lib.spk_schnet_scratch_floats(ctypes.byref(self.m), self.N)), dtype=torch.float32, device=dev)
        self.image = pack(self.w["in2f_w"], 0)

    def driver(self):
        """h_0 of one driver forward."""
        _lib, f = self._lib, self._lib.fptr

        def call():
            out = torch.empty(self.N, F, dtype=torch.float32, device=self.dev)
            saved = torch.full((self.n_saved,), float("nan"), dtype=torch.float32, device=self.dev)
            _lib.check(self.lib.spk_schnet_forward_f32(ctypes.byref(self.m), self.plan.graph(), ctypes.byref(self.rb), f(self.x0), f(self.r_ij), f(out), f(saved),
                                                       f(self.scratch), _lib.stream()))
            return saved
        return self.profiled(call)[:self.N * F].cpu()

    def comparator(self):
        _lib = self._lib
        h = torch.full((self.N, F), float("nan"), dtype=torch.float32, device=self.dev)
        c = chain_struct(_lib, self.N, self.x0, [dict(w=self.image, out=h, k=F, n_out=F, trans=2)])
        _lib.check(self.lib.spk_dense_chain_f32(ctypes.byref(c), _lib.stream()))
        torch.cuda.synchronize()
        return h.flatten().cpu()


class _Painn(_Box):
    def __init__(self, dev):
        super().__init__(dev)
        _lib = self._lib
        p = O.init_painn_params(n_interactions=1)
        a, x = "interactions.0.interatomic_context_net.", "mixing.0."
        t = {"ctx_w1": p[a + "0.weight"], "ctx_b1": p[a + "0.bias"], "ctx_w2": p[a + "1.weight"], "ctx_b2": p[a + "1.bias"],
             "filt_w": p["filter_net.weight"][:3 * F], "filt_b": p["filter_net.bias"][:3 * F], "mix_w": p[x + "mu_channel_mix.weight"],
             "ictx_w1": p[x + "intraatomic_context_net.0.weight"], "ictx_b1": p[x + "intraatomic_context_net.0.bias"],
             "ictx_w2": p[x + "intraatomic_context_net.1.weight"], "ictx_b2": p[x + "intraatomic_context_net.1.bias"]}
        t.update({k + "T": t[k].t() for k in ("ctx_w1", "ctx_w2", "mix_w", "ictx_w1", "ictx_w2")})
        self.w = {k: self.D(v) for k, v in t.items()}
        self.layers = (_lib.PainnLayerT * 1)()
        for k, v in self.w.items():
            setattr(self.layers[0], k, v.data_ptr())
        self.m = _lib.PainnT(F, 1, 1e-8, 0, self.layers, None)
        n_pack = int(self.lib.spk_painn_packed_floats(ctypes.byref(self.m)))
        assert n_pack > 0
        self.wpack = torch.empty(n_pack, dtype=torch.float32, device=dev)
        _lib.check(self.lib.spk_painn_pack_weights_f32(ctypes.byref(self.m), _lib.fptr(self.wpack), _lib.stream()))
        self.m.wpack = self.wpack.data_ptr()
        self.rb = self.radial(p)
        self.q0 = self.D(p["embedding.weight"][self.Z])
        self.n_saved = int(self.lib.spk_painn_saved_floats(ctypes.byref(self.m), self.N))
        self.scratch = torch.empty(int(self.lib.spk_painn_scratch_floats(ctypes.byref(self.m), self.N)), dtype=torch.float32, device=dev)
        self.images = (pack(self.w["ctx_w1"], 0), pack(self.w["ctx_w2"], 0))

    def driver(self):
        """preA_0 of one driver forward."""
        _lib, f = self._lib, self._lib.fptr

        def call():
            q = torch.empty(self.N, F, dtype=torch.float32, device=self.dev)
            mu = torch.empty(self.N, 3, F, dtype=torch.float32, device=self.dev)
            saved = torch.full((self.n_saved,), float("nan"), dtype=torch.float32, device=self.dev)
            _lib.check(self.lib.spk_painn_forward_f32(ctypes.byref(self.m), self.plan.graph(), ctypes.byref(self.rb), f(self.q0), f(self.r_ij), f(q), f(mu), f(saved),
                                                      f(self.scratch), _lib.stream()))
            return saved
        return self.profiled(call)[:self.N * F].cpu()

    def comparator(self):
        _lib = self._lib
        preA = torch.full((self.N, F), float("nan"), dtype=torch.float32, device=self.dev)
        c3 = torch.empty(self.N, 3 * F, dtype=torch.float32, device=self.dev)
        c = chain_struct(_lib, self.N, self.q0, [
            dict(w=self.images[0], b=self.w["ctx_b1"], pre_out=preA, k=F, n_out=F, act=_lib.SPK_ACT_SILU, trans=2),
            dict(w=self.images[1], b=self.w["ctx_b2"], out=c3, k=F, n_out=3 * F, trans=2)])
        _lib.check(self.lib.spk_dense_chain_f32(ctypes.byref(c), _lib.stream()))
        torch.cuda.synchronize()
        return preA.flatten().cpu()


@pytest.fixture(scope="module", params=["schnet", "painn"])
def case(request, dev):
    return request.param, (_Schnet if request.param == "schnet" else _Painn)(dev)


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_rows32_split_off_is_the_fp32_kernel(case):
    kind, c = case
    with _switches(32, False):
        drv, cmp = c.driver(), c.comparator()
    assert torch.isfinite(drv).all() and torch.isfinite(cmp).all()
    assert _same(drv, cmp), (kind, float((drv - cmp).abs().max()))


def test_rows32_split_on_is_the_split_kernel(case):
    kind, c = case
    with _switches(32, False):
        off = c.driver()
    with _switches(32, True):
        on = c.driver()
    assert torch.isfinite(on).all()
    n_diff = int((on.view(torch.int32) != off.view(torch.int32)).sum())
    err = float((on.double() - off.double()).abs().max() / off.double().abs().max())
    print("%s rows 32: split on against off: %d of %d elements differ, max |diff| / max |off| %.3e  (bound %.1e)" % (kind, n_diff, on.numel(), err, SPLIT_BOUND))
    assert n_diff >= 1
    assert err <= SPLIT_BOUND


def test_rows16_split_on_is_the_fp32_kernel(case):
    kind, c = case
    with _switches(16, True):
        drv, cmp = c.driver(), c.comparator()
    assert torch.isfinite(drv).all() and torch.isfinite(cmp).all()
    assert _same(drv, cmp), (kind, float((drv - cmp).abs().max()))


def test_no_state_crosses_calls(case):
    """The C-ABI chain gives the same bits before and right after a split-on driver forward on the same thread."""
    kind, c = case
    with _switches(32, True):
        before = c.comparator()
        c.driver()
        after = c.comparator()
    assert _same(before, after), (kind, float((before - after).abs().max()))
