"""Mirrors of ``schnetpack.nn.embedding`` (nn/embedding.py:158-349): ``NuclearEmbedding`` and ``ElectronicEmbedding`` with the reference's
constructors, buffers, parameter names and ``state_dict`` layout.

``ElectronicEmbedding`` spreads a molecule's total charge or spin multiplicity over its atoms by an attention-like block.  In eval mode on
float32 device tensors, for the shapes ``spk_eembed_supported`` covers (``num_features`` a multiple of 32 up to 256, up to four residual blocks,
shifted softplus or silu), it is ONE operator, ``torch.ops.spk_hip.electronic_embedding`` (three launches, csrc/spk_eembed.hip; no autograd node:
the embedding does not depend on the positions, so ``Forces`` needs no backward through it, and a backward into the output raises the eval-only
message).  Training mode, float64, host tensors and every other shape run the reference's formula on ATen -- the only route with parameter
gradients.
"""
import math
from typing import Callable, Dict, List, Union

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from .. import properties
from .. import torchops  # noqa: F401  (registers torch.ops.spk_hip)
from .activations import shifted_softplus
from .base import activation_id
from .blocks import ResidualMLP
from .fallback import note_fallback, use_aten

__all__ = ["NuclearEmbedding", "ElectronicEmbedding", "electron_config"]


def _electron_config_table() -> np.ndarray:
    """Ground-state electron configurations of Z = 0 .. 100, one row per element: Z, the occupations of 1s 2s 2p 3s 3p 4s 3d 4p 5s 4d 5p 6s 4f 5d
    6p 7s 5f 6d (in this filling order), then the valence occupations vs vp vd vf (what was filled since the last noble-gas core) -- the
    descriptor of the reference (nn/embedding.py:47-155), restated from the Madelung rule and the known exceptions, each column divided by its
    maximum."""
    order = ["1s", "2s", "2p", "3s", "3p", "4s", "3d", "4p", "5s", "4d", "5p", "6s", "4f", "5d", "6p", "7s", "5f", "6d"]
    cap = {"s": 2, "p": 6, "d": 10, "f": 14}
    # (shell that gives, shell that takes, electrons) against the filling order
    exceptions = {24: [("4s", "3d", 1)], 29: [("4s", "3d", 1)], 41: [("5s", "4d", 1)], 42: [("5s", "4d", 1)], 44: [("5s", "4d", 1)],
                  45: [("5s", "4d", 1)], 46: [("5s", "4d", 2)], 47: [("5s", "4d", 1)], 57: [("4f", "5d", 1)], 58: [("4f", "5d", 1)],
                  64: [("4f", "5d", 1)], 78: [("6s", "5d", 1)], 79: [("6s", "5d", 1)], 89: [("5f", "6d", 1)], 90: [("5f", "6d", 2)],
                  91: [("5f", "6d", 1)], 92: [("5f", "6d", 1)], 93: [("5f", "6d", 1)], 96: [("5f", "6d", 1)]}
    cores = [0, 2, 10, 18, 36, 54, 86]
    rows = []
    for z in range(101):
        occ = dict.fromkeys(order, 0)
        left = z
        for sh in order:
            n = min(left, cap[sh[1]])
            occ[sh] = n
            left -= n
        for giver, taker, n in exceptions.get(z, []):
            occ[giver] -= n
            occ[taker] += n
        core = max(c for c in cores if c < z) if z > 0 else 0
        val = {"s": 0, "p": 0, "d": 0, "f": 0}
        seen = 0
        for sh in order:      # shells past the core, in filling order
            full = cap[sh[1]]
            if seen >= core:
                val[sh[1]] += occ[sh]
            seen += full
        if z == 92:           # the reference's row of uranium lists its 5f3 6d1 valence as vd = 3, vf = 1; models were trained with it
            val["d"], val["f"] = 3, 1
        rows.append([z] + [occ[sh] for sh in order] + [val["s"], val["p"], val["d"], val["f"]])
    table = np.array(rows, dtype=np.float32)
    return table / np.max(table, axis=0)


electron_config = _electron_config_table()


class NuclearEmbedding(nn.Module):
    """Nuclear charge -> feature vector: a free table ``element_embedding`` [max_z, F] plus a linear map ``config_linear`` of the electron
    configuration.  Buffers: ``electron_config`` and the non-persistent ``embedding`` (the summed table), recomputed on every training-mode call
    and whenever the module switches to eval mode.  Like the reference's, only ``max_z == 101`` works (the configuration table has 101 rows); here
    any other value raises at construction."""

    def __init__(self, max_z: int, num_features: int, zero_init: bool = True):
        super().__init__()
        if max_z != electron_config.shape[0]:
            raise ValueError("NuclearEmbedding: max_z must be %d (the rows of the electron configuration table), got %d"
                             % (electron_config.shape[0], max_z))
        self.num_features = num_features
        self.register_buffer("electron_config", torch.tensor(electron_config))
        self.register_parameter("element_embedding", nn.Parameter(torch.empty(max_z, self.num_features)))
        self.register_buffer("embedding", torch.zeros(max_z, self.num_features), persistent=False)
        self.config_linear = nn.Linear(self.electron_config.size(1), self.num_features, bias=False)
        self.reset_parameters(zero_init)

    def reset_parameters(self, zero_init: bool = True) -> None:
        if zero_init:
            nn.init.zeros_(self.element_embedding)
            nn.init.zeros_(self.config_linear.weight)
        else:
            nn.init.uniform_(self.element_embedding, -math.sqrt(3), math.sqrt(3))
            nn.init.orthogonal_(self.config_linear.weight)

    def train(self, mode: bool = True):
        super().train(mode=mode)
        if not self.training:
            with torch.no_grad():
                self.embedding = self.element_embedding + self.config_linear(self.electron_config)
        return self

    def forward(self, atomic_numbers: torch.Tensor) -> torch.Tensor:
        if self.training:
            self.embedding = self.element_embedding + self.config_linear(self.electron_config)
        return self.embedding[atomic_numbers]


class ElectronicEmbedding(nn.Module):
    """Attention-like block that delocalises the molecular property ``inputs[property_key]`` (a charge when ``is_charged``: separate weights for
    its positive and negative part; else a spin: its magnitude) over the atoms of its molecule; returns the term that the representation adds to
    the nuclear embedding.  The number of molecules is the length of the property (the reference's ``len(inputs[idx])``, without that key)."""

    def __init__(self, property_key: str, num_features: int, is_charged: bool, num_residual: int = 1,
                 activation: Union[Callable, nn.Module] = shifted_softplus, epsilon: float = 1e-8):
        super().__init__()
        self.property_key = property_key
        self.is_charged = is_charged
        self.linear_q = nn.Linear(num_features, num_features)
        n_e = 2 if is_charged else 1
        self.linear_k = nn.Linear(n_e, num_features, bias=False)
        self.linear_v = nn.Linear(n_e, num_features, bias=False)
        self.resblock = ResidualMLP(num_features, num_residual, activation=activation, zero_init=True, bias=False)
        self.epsilon = epsilon
        self.reset_parameters()
        self._init_operator()

    def reset_parameters(self) -> None:
        nn.init.orthogonal_(self.linear_k.weight)
        nn.init.orthogonal_(self.linear_v.weight)
        nn.init.orthogonal_(self.linear_q.weight)
        nn.init.zeros_(self.linear_q.bias)

    def __setstate__(self, state):
        # instances restored from reference pickles never ran this __init__
        super().__setstate__(state)
        if "_act" not in self.__dict__:
            self._init_operator()

    def _init_operator(self) -> None:
        """``_act`` > 0: the activation id of the operator route; 0: the shape is declined (ATen).  ``force_aten`` keeps a covered shape on ATen."""
        act = activation_id(self.resblock.activation)
        stack = self.resblock.residual.stack
        plain = (self.linear_q.bias is not None and self.resblock.linear.bias is None
                 and all(b.linear1.bias is None and b.linear2.bias is None and b.activation1 is self.resblock.activation
                         and b.activation2 is self.resblock.activation for b in stack))
        ok = plain and act is not None and act != _lib.SPK_ACT_NONE
        if ok:
            ok = bool(_lib.lib().spk_eembed_supported(int(self.linear_q.in_features), len(stack), int(act)))
        self._act = int(act) if ok else 0
        self.force_aten = False

    def operator_weights(self) -> List[torch.Tensor]:
        ws = [self.linear_q.weight, self.linear_q.bias, self.linear_k.weight, self.linear_v.weight]
        for b in self.resblock.residual.stack:
            ws += [b.linear1.weight, b.linear2.weight]
        ws.append(self.resblock.linear.weight)
        return ws

    def on_operator(self, x: torch.Tensor, psi: torch.Tensor) -> bool:
        """Whether a call with these tensors takes ``torch.ops.spk_hip.electronic_embedding``."""
        return (self._act > 0 and not self.force_aten and not self.training and x.dim() == 2 and not use_aten(x) and not use_aten(psi)
                and not use_aten(self.linear_q.weight))

    def _operator(self, x: torch.Tensor, inputs: Dict[str, torch.Tensor], add_input: bool) -> torch.Tensor:
        y = torch.ops.spk_hip.electronic_embedding(x.detach(), inputs[self.property_key].detach(), inputs[properties.idx_m], self.operator_weights(),
                                                   self.is_charged, self._act, float(self.epsilon), add_input)
        if torch.is_grad_enabled():      # a backward pass into the eval-mode embedding gets the eval-only message, not silence
            y = torch.ops.spk_hip.eval_guard(y, [self.linear_q.weight])
        return y

    def add_to(self, x: torch.Tensor, inputs: Dict[str, torch.Tensor]) -> torch.Tensor:
        """``x + self(x, inputs)``; on the operator route the sum is formed in the kernel's epilogue."""
        if self.on_operator(x, inputs[self.property_key]):
            return self._operator(x, inputs, True)
        return x + self._aten(x, inputs)

    def forward(self, input_embedding: torch.Tensor, inputs: Dict[str, torch.Tensor]) -> torch.Tensor:
        if self.on_operator(input_embedding, inputs[self.property_key]):
            return self._operator(input_embedding, inputs, False)
        return self._aten(input_embedding, inputs)

    def _aten(self, input_embedding: torch.Tensor, inputs: Dict[str, torch.Tensor]) -> torch.Tensor:
        """The reference's formula (nn/embedding.py:311-349): a softmax over ALL atoms of the batch, renormalised per molecule."""
        note_fallback()
        idx_m = inputs[properties.idx_m]
        psi = inputs[self.property_key]
        num_batch = psi.shape[0]
        q = self.linear_q(input_embedding)
        if self.is_charged:
            e = F.relu(torch.stack([psi, -psi], dim=-1))
        else:
            e = torch.abs(psi).unsqueeze(-1)
        enorm = torch.maximum(e, torch.ones_like(e))
        k = self.linear_k(e / enorm)[idx_m]
        v = self.linear_v(e)[idx_m]
        weights = torch.sum(k * q, dim=-1) / k.shape[-1] ** 0.5
        a = F.softmax(weights, dim=0)
        anorm = a.new_zeros(num_batch).index_add_(0, idx_m, a)[idx_m]
        return self.resblock((a / (anorm + self.epsilon)).unsqueeze(-1) * v)


def embed_add(embedding: nn.Module, x: torch.Tensor, inputs: Dict[str, torch.Tensor]) -> torch.Tensor:
    """``x + embedding(x, inputs)`` for the ``embed()`` of the representations: a mirror on its operator route adds in the kernel, any other
    module is called as the reference calls it."""
    if type(embedding) is ElectronicEmbedding:
        return embedding.add_to(x, inputs)
    return x + embedding(x, inputs)
