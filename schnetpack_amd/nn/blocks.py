"""Mirrors of ``schnetpack.nn.blocks.build_mlp`` (nn/blocks.py:12-76), ``build_gated_equivariant_mlp`` (nn/blocks.py:79-156) and the residual
blocks ``Residual`` / ``ResidualStack`` / ``ResidualMLP`` (nn/blocks.py:159-296)."""
from typing import Callable, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F
from torch import nn

from .base import Dense
from .equivariant import GatedEquivariantBlock

__all__ = ["build_mlp", "build_gated_equivariant_mlp", "Residual", "ResidualStack", "ResidualMLP"]


def build_mlp(n_in: int, n_out: int, n_hidden: Optional[Union[int, Sequence[int]]] = None,
              n_layers: int = 2, activation: Callable = F.silu, last_bias: bool = True,
              last_zero_init: bool = False) -> nn.Module:
    if n_hidden is None:
        c = n_in
        sizes = []
        for _ in range(n_layers):
            sizes.append(c)
            c = max(n_out, c // 2)
        sizes.append(n_out)
    else:
        hidden = [n_hidden] * (n_layers - 1) if type(n_hidden) is int else list(n_hidden)
        sizes = [n_in] + hidden + [n_out]
    layers = [Dense(sizes[i], sizes[i + 1], activation=activation) for i in range(n_layers - 1)]
    if last_zero_init:
        layers.append(Dense(sizes[-2], sizes[-1], activation=None, weight_init=torch.nn.init.zeros_, bias=last_bias))
    else:
        layers.append(Dense(sizes[-2], sizes[-1], activation=None, bias=last_bias))
    return nn.Sequential(*layers)


class _GatedSequential(nn.Sequential):
    """``nn.Sequential`` over modules that map a (scalars, vectors) pair to such a pair, with the annotation TorchScript needs (the plain
    container's ``forward`` is inferred to take a tensor); same ``state_dict`` keys."""

    def forward(self, inputs: Tuple[torch.Tensor, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        for module in self:
            inputs = module(inputs)
        return inputs


def build_gated_equivariant_mlp(n_in: int, n_out: int, n_hidden: Optional[Union[int, Sequence[int]]] = None,
                                n_gating_hidden: Optional[Union[int, Sequence[int]]] = None, n_layers: int = 2,
                                activation: Callable = F.silu, sactivation: Callable = F.silu) -> nn.Module:
    """``n_layers`` ``GatedEquivariantBlock``s with the widths of :func:`build_mlp`; the gating networks are as wide as their block's
    input unless ``n_gating_hidden`` says otherwise, the last block has no scalar activation."""
    if n_hidden is None:
        c = n_in
        sizes = []
        for _ in range(n_layers):
            sizes.append(c)
            c = max(n_out, c // 2)
        sizes.append(n_out)
    else:
        hidden = [n_hidden] * (n_layers - 1) if type(n_hidden) is int else list(n_hidden)
        sizes = [n_in] + hidden + [n_out]
    if n_gating_hidden is None:
        gating = sizes[:-1]
    elif type(n_gating_hidden) is int:
        gating = [n_gating_hidden] * n_layers
    else:
        gating = list(n_gating_hidden)
    layers = [GatedEquivariantBlock(n_sin=sizes[i], n_vin=sizes[i], n_sout=sizes[i + 1], n_vout=sizes[i + 1], n_hidden=gating[i],
                                    activation=activation, sactivation=sactivation) for i in range(n_layers - 1)]
    layers.append(GatedEquivariantBlock(n_sin=sizes[-2], n_vin=sizes[-2], n_sout=sizes[-1], n_vout=sizes[-1], n_hidden=gating[-1],
                                        activation=activation, sactivation=None))
    return _GatedSequential(*layers)


class Residual(nn.Module):
    """Pre-activation residual block ``x + linear2(act(linear1(act(x))))``; ``linear1`` orthogonal, ``linear2`` zero (``zero_init``) or orthogonal,
    biases zero.  Plain ATen: the block carries the weights, the electronic embedding's operator runs them (``nn/embedding.py``)."""

    def __init__(self, num_features: int, activation: Union[Callable, nn.Module] = None, bias: bool = True, zero_init: bool = True) -> None:
        super().__init__()
        self.activation1 = activation
        self.linear1 = nn.Linear(num_features, num_features, bias=bias)
        self.activation2 = activation
        self.linear2 = nn.Linear(num_features, num_features, bias=bias)
        self.reset_parameters(bias, zero_init)

    def reset_parameters(self, bias: bool = True, zero_init: bool = True) -> None:
        nn.init.orthogonal_(self.linear1.weight)
        if zero_init:
            nn.init.zeros_(self.linear2.weight)
        else:
            nn.init.orthogonal_(self.linear2.weight)
        if bias:
            nn.init.zeros_(self.linear1.bias)
            nn.init.zeros_(self.linear2.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x + self.linear2(self.activation2(self.linear1(self.activation1(x))))


class ResidualStack(nn.Module):
    """``num_residual`` :class:`Residual` blocks in sequence (``stack``)."""

    def __init__(self, num_features: int, num_residual: int, activation: Union[Callable, nn.Module], bias: bool = True, zero_init: bool = True) -> None:
        super().__init__()
        self.stack = nn.ModuleList([Residual(num_features, activation, bias, zero_init) for _ in range(num_residual)])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        for residual in self.stack:
            x = residual(x)
        return x


class ResidualMLP(nn.Module):
    """``linear(act(residual(x)))``: a :class:`ResidualStack` (always zero-initialised, like the reference's) and an output layer that is
    orthogonal or, with ``zero_init``, zero."""

    def __init__(self, num_features: int, num_residual: int, activation: Union[Callable, nn.Module], bias: bool = True, zero_init: bool = False):
        super().__init__()
        self.residual = ResidualStack(num_features, num_residual, activation=activation, bias=bias, zero_init=True)
        self.linear = nn.Linear(num_features, num_features, bias=bias)
        self.activation = activation
        self.reset_parameters(bias, zero_init)

    def reset_parameters(self, bias: bool = True, zero_init: bool = False) -> None:
        if zero_init:
            nn.init.zeros_(self.linear.weight)
        else:
            nn.init.orthogonal_(self.linear.weight)
        if bias:
            nn.init.zeros_(self.linear.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.linear(self.activation(self.residual(x)))
