"""Mirror of ``schnetpack.nn.so3`` (nn/so3.py:18-357, nn/ops/so3.py:9-21): same class names, constructors, buffers (names and persistence) and
``state_dict`` keys, on the SO(3) kernels of csrc/spk_so3.hip.

Eval mode, float32 tensors on the device, ``1 <= lmax <= 3``, a feature width the kernels take (a multiple of 32 up to 256) and -- for the
convolution -- a neighbour list sorted by ``idx_i`` and symmetric: ``RealSphericalHarmonics`` is ``torch.ops.spk_hip.real_sph_harm``,
``SO3Convolution`` is the filter network (the ``dense`` operator) followed by ONE ``torch.ops.spk_hip.so3_conv`` -- the reference's gathered
``[n_pairs, n_cg, F]`` tensors (83 F floats per pair at ``lmax = 2``, 353 F at ``lmax = 3``) never exist -- and ``SO3TensorProduct`` is
``torch.ops.spk_hip.so3_product``.  The operators return first-order gradients (what ``Forces`` asks for); a recorded backward raises the eval-only
message.  Everything else -- training mode, float64, host tensors, ``lmax`` 0 or above 3, other widths, other lists -- runs the reference's
formula on ATen (``nn/fallback.py``), differentiable to any order.  The gates multiply by ``sigmoid`` on ATen elementwise kernels; their
``scaling`` layer is the ``dense`` operator.

The Clebsch-Gordan table comes from ``nn/so3_tables.py`` (exact closed form, the reference's real-basis convention and non-zero order), cast to
float32 like the reference's buffer.
"""
import math
from functools import lru_cache
from typing import Tuple

import torch
import torch.nn as nn

from .. import torchops  # noqa: F401  (registers torch.ops.spk_hip)
from . import so3_tables
from .base import Dense
from .fallback import note_fallback, use_aten
from .scatter import scatter_add

__all__ = ["RealSphericalHarmonics", "scalar2rsh", "SO3TensorProduct", "SO3Convolution", "SO3ParametricGatedNonlinearity", "SO3GatedNonlinearity",
           "sh_indices", "so3_kernel_shape"]


@lru_cache(maxsize=10)
def sh_indices(lmax: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(l, m) of every combined index s = l^2 + l + m, as two int64 tensors."""
    l, m = so3_tables.sh_lm(int(lmax))
    return torch.from_numpy(l.astype("int64")), torch.from_numpy(m.astype("int64"))


def so3_kernel_shape(lmax: int, n_features: int) -> bool:
    """True for the shapes the kernels are instantiated for."""
    return 1 <= int(lmax) <= so3_tables.LMAX_KERNEL and 32 <= int(n_features) <= 256 and int(n_features) % 32 == 0


def _device_route(module: nn.Module, *tensors: torch.Tensor) -> bool:
    """Eval mode and every tensor float32 on the device (or meta)."""
    if module.training:
        return False
    dev = tensors[0].device
    return all((not use_aten(t)) and t.device == dev for t in tensors)


def _cg_buffers(module: nn.Module, lmax: int):
    v, i1, i2, io = so3_tables.cg_sparse(int(lmax))
    module.register_buffer("idx_in_1", torch.from_numpy(i1.astype("int64")), persistent=False)
    module.register_buffer("idx_in_2", torch.from_numpy(i2.astype("int64")), persistent=False)
    module.register_buffer("idx_out", torch.from_numpy(io.astype("int64")), persistent=False)
    module.register_buffer("clebsch_gordan", torch.from_numpy(v.astype("float32")), persistent=False)


class RealSphericalHarmonics(nn.Module):
    """Real spherical harmonics of a batch of vectors up to ``lmax``, ordered (l, m) = (0, 0), (1, -1), (1, 0), (1, 1), (2, -2), ...;
    Y_lm = N_l Pi_l^|m|(z) AB_m(x, y) with x, y, z taken as they come (unit vectors are the caller's business, as in the reference)."""

    def __init__(self, lmax: int, dtype_str: str = "float32"):
        super().__init__()
        self.lmax = lmax
        dtype = getattr(torch, dtype_str.split(".")[-1]) if isinstance(dtype_str, str) else dtype_str
        _, pi, zpow, a, b = so3_tables.rsh_coefficients(int(lmax))
        m, p = torch.broadcast_tensors(torch.arange(1, lmax + 1, dtype=torch.float64)[:, None], torch.arange(0, lmax + 1, dtype=torch.float64)[None, :])
        powers = torch.stack([p, m - p], dim=-1) * (p <= m)[:, :, None]      # exponents of x and y in the terms of A_m / B_m
        a_t, b_t = torch.from_numpy(a[:lmax].copy()), torch.from_numpy(b[:lmax].copy())
        self.register_buffer("powers", powers.to(dtype=dtype), False)
        self.register_buffer("zpow", torch.from_numpy(zpow.astype("float64")).to(dtype=dtype), False)
        self.register_buffer("cAm", a_t.to(dtype=dtype), False)
        self.register_buffer("cBm", b_t.to(dtype=dtype), False)
        self.register_buffer("cPi", torch.from_numpy(pi.copy()).to(dtype=dtype), False)
        self.lidx, self.midx = sh_indices(lmax)
        self.register_buffer("flidx", self.lidx.to(dtype=dtype), False)

    def _aten(self, directions: torch.Tensor) -> torch.Tensor:
        lmax = int(self.lmax)
        x, y, z = directions[:, 0], directions[:, 1], directions[:, 2]
        one = torch.ones_like(x)

        def powers_of(v):      # v^0 .. v^lmax by products: a zero exponent never meets the base (no 0 * inf in the gradient)
            out = [one]
            for _ in range(lmax):
                out.append(out[-1] * v)
            return out

        xp, yp, zp = powers_of(x), powers_of(y), powers_of(z)
        _, pi_t, zpow_t, a_t, b_t = so3_tables.rsh_coefficients(lmax)
        A, B = [None], [None]
        for m in range(1, lmax + 1):
            am = sum(self.cAm[m - 1, p] * xp[p] * yp[m - p] for p in range(m + 1) if a_t[m - 1, p] != 0.0)
            bm = sum(self.cBm[m - 1, p] * xp[p] * yp[m - p] for p in range(m + 1) if b_t[m - 1, p] != 0.0)
            A.append(am)
            B.append(bm)
        cols = []
        for l, m in zip(self.lidx.tolist(), self.midx.tolist()):
            am = abs(m)
            pi = sum(self.cPi[l, am, k] * zp[int(zpow_t[l, am, k])] for k in range((l - am) // 2 + 1))
            ab = math.sqrt(0.5) * one if m == 0 else (A[m] if m > 0 else B[am])
            cols.append(math.sqrt((2 * l + 1) / (2 * math.pi)) * pi * ab)
        return torch.stack(cols, dim=1)

    def forward(self, directions: torch.Tensor) -> torch.Tensor:
        if _device_route(self, directions) and 1 <= int(self.lmax) <= so3_tables.LMAX_KERNEL and directions.dim() == 2:
            return torch.ops.spk_hip.real_sph_harm(directions, int(self.lmax))
        note_fallback()
        return self._aten(directions)


def scalar2rsh(x: torch.Tensor, lmax: int) -> torch.Tensor:
    """Zero-pad scalar features [N, 1, F] to [N, (lmax+1)^2, F]."""
    pad = torch.zeros((x.shape[0], int((lmax + 1) ** 2 - 1), x.shape[2]), device=x.device, dtype=x.dtype)
    return torch.cat([x, pad], dim=1)


class SO3TensorProduct(nn.Module):
    r"""Clebsch-Gordan tensor product y_{s,f} = \sum_{s1,s2} C_{s1,s2}^{s} x1_{s1,f} x2_{s2,f}."""

    def __init__(self, lmax: int):
        super().__init__()
        self.lmax = lmax
        _cg_buffers(self, lmax)

    def forward(self, x1: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
        if _device_route(self, x1, x2) and x1.dim() == 3 and x1.shape == x2.shape and so3_kernel_shape(self.lmax, x1.shape[2]):
            return torch.ops.spk_hip.so3_product(x1, x2, int(self.lmax))
        note_fallback()
        y = x1[:, self.idx_in_1, :] * x2[:, self.idx_in_2, :] * self.clebsch_gordan[None, :, None]
        return scatter_add(y, self.idx_out, dim_size=int((self.lmax + 1) ** 2), dim=1)


class SO3Convolution(nn.Module):
    r"""Clebsch-Gordan convolution y_{i,s,f} = \sum_{j,s1,s2} x_{j,s2,f} W_{s1,f}(r_ij) Y_{s1}(r_ij) C_{s1,s2}^{s}."""

    def __init__(self, lmax: int, n_atom_basis: int, n_radial: int):
        super().__init__()
        self.lmax = lmax
        self.n_atom_basis = n_atom_basis
        self.n_radial = n_radial
        _cg_buffers(self, lmax)
        self.filternet = Dense(n_radial, n_atom_basis * (self.lmax + 1), activation=None)
        lidx, _ = sh_indices(lmax)
        self.register_buffer("Widx", lidx[self.idx_in_1])

    def _compute_radial_filter(self, radial_ij: torch.Tensor, cutoff_ij: torch.Tensor) -> torch.Tensor:
        """Radial filters [n_neighbors, n_clebsch_gordan, n_features] (the reference's materialised form; the device route never builds it)."""
        Wij = self.filternet(radial_ij) * cutoff_ij
        Wij = torch.reshape(Wij, (-1, self.lmax + 1, self.n_atom_basis))
        return Wij[:, self.Widx]

    def _kernel_route(self, x, radial_ij, dir_ij, cutoff_ij, idx_i, idx_j) -> bool:
        if not (_device_route(self, x, radial_ij, dir_ij, cutoff_ij) and x.dim() == 3 and so3_kernel_shape(self.lmax, x.shape[2])):
            return False
        P = idx_i.shape[0]
        if not (x.shape[2] == self.n_atom_basis and dir_ij.dim() == 2 and dir_ij.shape[0] == P and cutoff_ij.numel() == P):
            return False
        if x.is_meta:
            return True
        return bool(torch.ops.spk_hip.so3_list_ok(dir_ij.detach(), cutoff_ij.detach(), idx_i, idx_j, int(x.shape[0])))

    def forward(self, x: torch.Tensor, radial_ij: torch.Tensor, dir_ij: torch.Tensor, cutoff_ij: torch.Tensor, idx_i: torch.Tensor,
                idx_j: torch.Tensor) -> torch.Tensor:
        if self._kernel_route(x, radial_ij, dir_ij, cutoff_ij, idx_i, idx_j):
            W = self.filternet(radial_ij)
            return torch.ops.spk_hip.so3_conv(x, W, dir_ij, cutoff_ij, idx_i, idx_j, int(self.lmax))
        note_fallback()
        xj = x[idx_j[:, None], self.idx_in_2[None, :], :]
        Wij = self._compute_radial_filter(radial_ij, cutoff_ij)
        v = Wij * dir_ij[:, self.idx_in_1, None] * self.clebsch_gordan[None, :, None] * xj
        yij = scatter_add(v, self.idx_out, dim_size=int((self.lmax + 1) ** 2), dim=1)
        return scatter_add(yij, idx_i, dim_size=x.shape[0])


def linear(layer: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    """An ``nn.Linear`` of the reference's layout through the ``dense`` operator (on the [N S, F] view) when the tensor is on the device."""
    if use_aten(x):
        return layer(x)
    return torch.ops.spk_hip.dense(x, layer.weight, layer.bias, 0)


class SO3ParametricGatedNonlinearity(nn.Module):
    r"""y_{i,s,f} = x_{i,s,f} \sigma(f(x_{i,0,\cdot}))_{l(s),f} with a learned linear map f."""

    def __init__(self, n_in: int, lmax: int):
        super().__init__()
        self.lmax = lmax
        self.n_in = n_in
        self.lidx, _ = sh_indices(lmax)
        self.scaling = nn.Linear(n_in, n_in * (lmax + 1))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        s0 = x[:, 0, :]
        h = linear(self.scaling, s0).reshape(-1, self.lmax + 1, self.n_in)
        h = torch.cat([h[:, l:l + 1].expand(-1, 2 * l + 1, -1) for l in range(int(self.lmax) + 1)], dim=1)      # h[:, l(s)] without an index tensor
        return x * torch.sigmoid(h)


class SO3GatedNonlinearity(nn.Module):
    r"""y_{i,s,f} = x_{i,s,f} \sigma(x_{i,0,f})."""

    def __init__(self, lmax: int):
        super().__init__()
        self.lmax = lmax
        self.lidx, _ = sh_indices(lmax)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        s0 = x[:, 0, :]
        return x * torch.sigmoid(s0[:, None, :])
