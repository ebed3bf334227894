"""ctypes helpers of the fused Dense chain (spk_dense_chain_f32) shared by test_gpu_ops.py and test_gpu_chain_route.py."""
import torch


def chain_struct(_lib, m, inp, layers, in_pre=None, in_act=0, zero=None, tmp=None):
    c = _lib.ChainT()
    c.n_layers = len(layers)
    c.in_act = in_act
    c.m = m
    c.inp = _lib.fptr(inp)
    c.in_pre = _lib.fptr(in_pre)
    c.zero_ptr = _lib.fptr(zero)
    c.zero_count = zero.numel() if zero is not None else 0
    if tmp is not None:
        c.tmp[0] = tmp[0].data_ptr()
        c.tmp[1] = tmp[1].data_ptr()
    for l, L in enumerate(layers):
        for k in ("w", "b", "res", "out", "pre_out", "post_pre"):
            setattr(c.layers[l], k, _lib.fptr(L.get(k)))
        for k in ("k", "n_out", "act", "trans", "post_act"):
            setattr(c.layers[l], k, int(L.get(k, 0)))
    return c


def pack(w, transposed):
    """spk_pack_weight_f32 image of a Linear weight [n_out, k_in] (device tensor)."""
    from schnetpack_amd import _lib
    P = torch.empty(w.numel(), device=w.device)
    _lib.check(_lib.lib().spk_pack_weight_f32(_lib.fptr(w), w.shape[0], w.shape[1], transposed, _lib.fptr(P), _lib.stream()))
    return P
