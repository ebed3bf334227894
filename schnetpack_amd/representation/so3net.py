"""Mirror of ``schnetpack.representation.so3net.SO3net`` (representation/so3net.py:15-155): same constructor, attributes, ``state_dict`` keys and
outputs (``scalar_representation``, ``multipole_representation``, with ``return_vector_representation`` also ``vector_representation``).

Module by module on the SO(3) operators (nn/so3.py).  In eval mode on float32 device tensors the forward of one interaction is seven operator
launches -- filter network (``dense``), ``so3_conv``, mixing 1 (``dense``), ``so3_product``, mixing 2 (``dense``), the gate's ``scaling`` (``dense``),
mixing 3 (``dense``) -- and five ATen elementwise kernels (two adds, and the gate's expand, sigmoid and multiply); no tensor larger than the filter
[n_pairs, (lmax+1) F] exists.  ``Forces`` gets dE/dR (and dE/dstrain through ``Strain``) from the operators' first-order backward.  Training mode,
float64 and host tensors take the ATen route of every layer.
"""
from typing import Callable, Dict, List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import properties
from .. import torchops  # noqa: F401  (registers torch.ops.spk_hip)
from ..nn import replicate_module
from ..nn import so3
from ..nn.embedding import embed_add
from ..nn.fallback import use_aten

__all__ = ["SO3net"]


class SO3net(nn.Module):
    """SO(3)-equivariant representation from spherical harmonics and Clebsch-Gordan tensor products."""

    def __init__(self, n_atom_basis: int, n_interactions: int, lmax: int, radial_basis: nn.Module, cutoff_fn: Optional[Callable] = None,
                 shared_interactions: bool = False, return_vector_representation: bool = False, activation: Optional[Callable] = F.silu,
                 nuclear_embedding: Optional[nn.Module] = None, electronic_embeddings: Optional[List] = None):
        super().__init__()
        self.n_atom_basis = n_atom_basis
        self.n_interactions = n_interactions
        self.lmax = lmax
        self.cutoff_fn = cutoff_fn
        self.cutoff = cutoff_fn.cutoff
        self.radial_basis = radial_basis
        self.return_vector_representation = return_vector_representation
        self.activation = activation

        if nuclear_embedding is None:
            nuclear_embedding = nn.Embedding(100, n_atom_basis)
        self.embedding = nuclear_embedding
        if electronic_embeddings is None:
            electronic_embeddings = []
        self.electronic_embeddings = nn.ModuleList(electronic_embeddings)

        self.sphharm = so3.RealSphericalHarmonics(lmax=lmax)
        self.so3convs = replicate_module(lambda: so3.SO3Convolution(lmax, n_atom_basis, self.radial_basis.n_rbf), self.n_interactions,
                                         shared_interactions)
        self.mixings1 = replicate_module(lambda: nn.Linear(n_atom_basis, n_atom_basis, bias=False), self.n_interactions, shared_interactions)
        self.mixings2 = replicate_module(lambda: nn.Linear(n_atom_basis, n_atom_basis, bias=False), self.n_interactions, shared_interactions)
        self.mixings3 = replicate_module(lambda: nn.Linear(n_atom_basis, n_atom_basis, bias=False), self.n_interactions, shared_interactions)
        self.gatings = replicate_module(lambda: so3.SO3ParametricGatedNonlinearity(n_atom_basis, lmax), self.n_interactions, shared_interactions)
        self.so3product = so3.SO3TensorProduct(lmax)

    def embed(self, inputs: Dict[str, torch.Tensor]) -> torch.Tensor:
        """x_0: nuclear embedding rows plus the electronic embeddings (so3net.py:130-132)."""
        x0 = self.embedding(inputs[properties.Z])
        for embedding in self.electronic_embeddings:      # a mirror on its operator route adds x0 in the kernel's epilogue
            x0 = embed_add(embedding, x0, inputs)
        return x0

    def forward(self, inputs: Dict[str, torch.Tensor]):
        atomic_numbers = inputs[properties.Z]
        r_ij = inputs[properties.Rij]
        idx_i = inputs[properties.idx_i]
        idx_j = inputs[properties.idx_j]

        if not self.training and r_ij.is_cuda and not use_aten(r_ij) and idx_i.shape[0] > 0:
            # the plan of the list from its true geometry (cached on the index tensors): the convolutions find the reverse-edge map there
            torch.ops.spk_hip.edge_plan(idx_i, idx_j, int(atomic_numbers.shape[0]), r_ij.detach(), 0.0, -1)

        d_ij = torch.norm(r_ij, dim=1, keepdim=True)
        dir_ij = r_ij / d_ij

        Yij = self.sphharm(dir_ij)
        radial_ij = self.radial_basis(d_ij)
        cutoff_ij = self.cutoff_fn(d_ij)[..., None]

        x0 = self.embed(inputs).unsqueeze(1)

        x = so3.scalar2rsh(x0, int(self.lmax))
        for so3conv, mixing1, mixing2, gating, mixing3 in zip(self.so3convs, self.mixings1, self.mixings2, self.gatings, self.mixings3):
            dx = so3conv(x, radial_ij, Yij, cutoff_ij, idx_i, idx_j)
            ddx = so3.linear(mixing1, dx)
            dx = dx + self.so3product(dx, ddx)
            dx = so3.linear(mixing2, dx)
            dx = gating(dx)
            dx = so3.linear(mixing3, dx)
            x = x + dx

        inputs["scalar_representation"] = x[:, 0]
        inputs["multipole_representation"] = x
        if self.return_vector_representation:      # l = 1 features from (y, z, x) to Cartesian (x, y, z) order
            inputs["vector_representation"] = torch.roll(x[:, 1:4], 1, 1)
        return inputs
