"""Mirror of ``schnetpack.nn.equivariant.GatedEquivariantBlock`` (nn/equivariant.py:11-71)."""
from typing import Callable, Final, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from .base import Dense

__all__ = ["GatedEquivariantBlock"]


class GatedEquivariantBlock(nn.Module):
    """Gated equivariant block: ``[V | W] = mix_vectors(v)``, ``x = scalar_net([s | |V|])``, ``s' = sactivation(x[:n_sout])``,
    ``v' = x[n_sout:] * W``.  Same constructor, attributes and ``state_dict`` keys (``mix_vectors.weight``, ``scalar_net.{0,1}.{weight,bias}``)
    as the reference.  The block itself is the reference's formula on the ``Dense`` mirrors (any device and dtype, parameter gradients);
    a whole stack of them behind a ``DipoleMoment`` / ``Polarizability`` head runs as ONE kernel in eval mode
    (``torch.ops.spk_hip.gated_mlp``, see :mod:`schnetpack_amd.atomistic`)."""

    _has_sact: Final[bool]

    def __init__(self, n_sin: int, n_vin: int, n_sout: int, n_vout: int, n_hidden: int, activation: Callable = F.silu,
                 sactivation: Optional[Callable] = None):
        super().__init__()
        self.n_sin = n_sin
        self.n_vin = n_vin
        self.n_sout = n_sout
        self.n_vout = n_vout
        self.n_hidden = n_hidden
        self.mix_vectors = Dense(n_vin, 2 * n_vout, activation=None, bias=False)
        self.scalar_net = nn.Sequential(
            Dense(n_sin + n_vout, n_hidden, activation=activation),
            Dense(n_hidden, n_sout + n_vout, activation=None),
        )
        self.sactivation = sactivation
        self._has_sact = sactivation is not None

    def __setstate__(self, state):
        # instances restored from reference pickles never ran this __init__
        super().__setstate__(state)
        if "_has_sact" not in self.__dict__:
            self._has_sact = self.__dict__.get("sactivation") is not None

    def forward(self, inputs: Tuple[torch.Tensor, torch.Tensor]):
        scalars, vectors = inputs
        vmix = self.mix_vectors(vectors)
        vectors_V, vectors_W = torch.split(vmix, self.n_vout, dim=-1)
        vectors_Vn = torch.norm(vectors_V, dim=-2)
        ctx = torch.cat([scalars, vectors_Vn], dim=-1)
        x = self.scalar_net(ctx)
        s_out, x = torch.split(x, [self.n_sout, self.n_vout], dim=-1)
        v_out = x.unsqueeze(-2) * vectors_W
        if self._has_sact:
            s_out = self.sactivation(s_out)
        return s_out, v_out
