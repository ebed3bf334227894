"""Mirrors of the reference *callers* either side of the hot path, so that a complete force call can be
assembled (and scripted) without the reference package: ``Strain`` (atomistic/response.py:434-464), ``PairwiseDistances``
(atomistic/distances.py:9-26), ``Atomwise`` (atomistic/atomwise.py:14-88) and ``Forces`` (atomistic/response.py:18-92).  In an integration the
reference's own modules run unchanged on top of the HIP classes (tests/test_gpu_reference_callers.py) -- they only see
``schnetpack.nn.scatter_add`` / ``Dense`` / the representation classes; ``install(fused_head=True)`` swaps in this
``Atomwise`` for its one-kernel energy head.  ``ZBLRepulsionEnergy`` (atomistic/nuclear_repulsion.py:13-108) and ``Aggregation``
(atomistic/aggregation.py:9-28) add the short-range nuclear repulsion production potentials carry next to the learned energy.
"""
from typing import Callable, Dict, Final, List, Optional, Sequence, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, properties
from . import units as spk_units
from . import torchops  # noqa: F401  (registers torch.ops.spk_hip)
from .nn import CosineCutoff, Dense, build_mlp, scatter_add
from .nn.base import activation_id
from .nn.fallback import note_fallback, use_aten

__all__ = ["Strain", "PairwiseDistances", "Atomwise", "Forces", "ZBLRepulsionEnergy", "Aggregation"]


class Strain(nn.Module):
    """Zero strain S [n_mol, 3, 3] (requires grad) applied to positions, offsets and cell as x (1 + S^T), so that ``Forces(calc_stress=True)``
    can differentiate the energy w.r.t. it.  Module by module this is the reference's formula on any device and dtype; the standard
    potential with stress (``model.classify_potential`` == 3) does not run it: its operator returns dE/dS directly."""

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        strain = torch.zeros_like(inputs[properties.cell])
        strain.requires_grad_()
        inputs[properties.strain] = strain
        strain = strain.transpose(1, 2)
        inputs[properties.cell] = inputs[properties.cell] + torch.matmul(inputs[properties.cell], strain)
        idx_m = inputs[properties.idx_m]
        strain_i = strain[idx_m]
        inputs[properties.R] = inputs[properties.R] + torch.matmul(inputs[properties.R][:, None, :], strain_i).squeeze(1)
        idx_i = inputs[properties.idx_i]
        strain_ij = strain_i[idx_i]
        inputs[properties.offsets] = inputs[properties.offsets] + torch.matmul(inputs[properties.offsets][:, None, :], strain_ij).squeeze(1)
        return inputs


class PairwiseDistances(nn.Module):
    """Rij = R[idx_j] - R[idx_i] + offsets; autograd lands dE/dRij back on the atoms (segmented row sum on
    sorted symmetric lists) and on the offsets (stress via ``Strain``)."""

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        R = inputs[properties.R]
        offsets: Optional[torch.Tensor] = None
        if properties.offsets in inputs:
            offsets = inputs[properties.offsets]
        idx_i = inputs[properties.idx_i]
        idx_j = inputs[properties.idx_j]
        if use_aten(R):          # host / non-float32 tensors: the reference's formula (atomistic/distances.py:19-25)
            note_fallback()
            Rij = R[idx_j] - R[idx_i]
            inputs[properties.Rij] = Rij + offsets if offsets is not None else Rij
            return inputs
        inputs[properties.Rij] = torch.ops.spk_hip.pairwise(R, idx_i, idx_j, offsets)
        return inputs


class Atomwise(nn.Module):
    """Per-atom MLP + sum over ``idx_m`` (aggregation_mode 'sum' / 'avg' / None).  In eval mode the default head
    (2 layers, width-1 output) is ONE kernel each way (``torch.ops.spk_hip.atomwise``)."""

    _fused_head: Final[bool]

    def __init__(self, n_in: int, n_out: int = 1, n_hidden: Optional[Union[int, Sequence[int]]] = None,
                 n_layers: int = 2, activation: Callable = F.silu, aggregation_mode: str = "sum",
                 output_key: str = "y", per_atom_output_key: Optional[str] = None,
                 n_molecules_key: str = "_n_molecules"):
        super().__init__()
        self.output_key = output_key
        self.model_outputs = [output_key]
        self.per_atom_output_key = per_atom_output_key
        if per_atom_output_key is not None:
            self.model_outputs.append(per_atom_output_key)
        self.n_out = n_out
        if aggregation_mode is None and per_atom_output_key is None:
            raise ValueError("If `aggregation_mode` is None, `per_atom_output_key` needs to be set,"
                             " since no accumulated output will be returned!")
        self.outnet = build_mlp(n_in=n_in, n_out=n_out, n_hidden=n_hidden, n_layers=n_layers,
                                activation=activation)
        self.aggregation_mode = aggregation_mode
        self.n_molecules_key = n_molecules_key
        self._head_act = 0
        self._fused_head = self._head_fusable()

    def __setstate__(self, state):
        # a model pickled by the REFERENCE (torch.save(model), task.py:300) unpickled onto this class after
        # install(fused_head=True) never ran __init__: fill what the reference's Atomwise does not carry
        super().__setstate__(state)
        if "n_molecules_key" not in self.__dict__:
            self.n_molecules_key = "_n_molecules"
        if "_fused_head" not in self.__dict__ or "_head_act" not in self.__dict__:
            self._head_act = 0
            self._fused_head = self._head_fusable()

    def _head_fusable(self) -> bool:
        """True when the head is the default 2-layer / width-1 MLP the fused HIP kernel covers."""
        if self.aggregation_mode is None or self.n_out != 1:
            return False
        net = self.outnet
        if not (isinstance(net, nn.Sequential) and len(net) == 2 and all(isinstance(l, Dense) for l in net)):
            return False
        act = activation_id(net[0].activation)
        if act is None or act == _lib.SPK_ACT_NONE or activation_id(net[1].activation) != _lib.SPK_ACT_NONE:
            return False
        if net[1].out_features != 1 or net[0].bias is None or net[1].bias is None:
            return False
        if not bool(_lib.lib().spk_atomwise_supported(int(net[0].in_features), int(net[0].out_features), int(act))):
            return False
        self._head_act = int(act)
        return True

    def _n_molecules(self, inputs: Dict[str, torch.Tensor], idx_m: torch.Tensor) -> int:
        # the reference reads int(idx_m[-1]) + 1 (a device sync, atomwise.py:80); a host-side molecule count in the
        # batch dict (python int or CPU tensor under `n_molecules_key`) avoids it when present
        if self.n_molecules_key in inputs:
            return int(inputs[self.n_molecules_key])
        return int(idx_m[-1]) + 1

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        x = inputs["scalar_representation"]
        if self._fused_head and not self.training and x.dim() == 2 and not use_aten(x):
            idx_m = inputs[properties.idx_m]
            maxm = self._n_molecules(inputs, idx_m)
            l0 = self.outnet[0]
            l1 = self.outnet[1]
            y, y_atom = torch.ops.spk_hip.atomwise(x, l0.weight, l0.bias, l1.weight, l1.bias, idx_m, maxm, self._head_act)
            if self.per_atom_output_key is not None:
                inputs[self.per_atom_output_key] = y_atom
            if self.aggregation_mode == "avg":
                y = y / inputs[properties.n_atoms]
            inputs[self.output_key] = y
            return inputs
        y = self.outnet(x)
        if self.per_atom_output_key is not None:
            inputs[self.per_atom_output_key] = y
        if self.aggregation_mode is not None:
            idx_m = inputs[properties.idx_m]
            maxm = self._n_molecules(inputs, idx_m)
            y = scatter_add(y, idx_m, dim_size=maxm)
            y = torch.squeeze(y, -1)
            if self.aggregation_mode == "avg":
                y = y / inputs[properties.n_atoms]
        inputs[self.output_key] = y
        return inputs


class Forces(nn.Module):
    """forces = -dE/dR (and stress = dE/dstrain / volume) by autograd, ``create_graph = training``, like the reference."""

    def __init__(self, calc_forces: bool = True, calc_stress: bool = False, energy_key: str = properties.energy,
                 force_key: str = properties.forces, stress_key: str = properties.stress):
        super().__init__()
        self.calc_forces = calc_forces
        self.calc_stress = calc_stress
        self.energy_key = energy_key
        self.force_key = force_key
        self.stress_key = stress_key
        self.model_outputs = []
        if calc_forces:
            self.model_outputs.append(force_key)
        if calc_stress:
            self.model_outputs.append(stress_key)
        self.required_derivatives = []
        if calc_forces:
            self.required_derivatives.append(properties.R)
        if calc_stress:
            self.required_derivatives.append(properties.strain)

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        Epred = inputs[self.energy_key]
        go: List[Optional[torch.Tensor]] = [torch.ones_like(Epred)]
        grads = torch.autograd.grad([Epred], [inputs[prop] for prop in self.required_derivatives],
                                    grad_outputs=go, create_graph=self.training)
        if self.calc_forces:
            dEdR = grads[0]
            if dEdR is None:
                dEdR = torch.zeros_like(inputs[properties.R])
            inputs[self.force_key] = -dEdR
        if self.calc_stress:
            stress = grads[-1]
            if stress is None:
                stress = torch.zeros_like(inputs[properties.cell])
            cell = inputs[properties.cell]
            volume = torch.sum(cell[:, 0, :] * torch.cross(cell[:, 1, :], cell[:, 2, :], dim=1), dim=1, keepdim=True)[:, :, None]
            inputs[self.stress_key] = stress / volume
        return inputs


def _softplus_inverse(x: torch.Tensor) -> torch.Tensor:
    """y with softplus(y) = x (nn/activations.py:25-35)."""
    return x + torch.log(-torch.expm1(-x))


class ZBLRepulsionEnergy(nn.Module):
    """Ziegler-Biersack-Littmark style nuclear repulsion, the reference's formula (atomistic/nuclear_repulsion.py:70-108):
    ``a_z = z^p``, ``a_ij = (a_zi + a_zj) s``, ``phi = sum_k c_k exp(-a_ij alpha_k d)``, ``E = 1/2 ke sum_pairs z_i z_j phi f_c / d``.
    Constructor, parameters (``a_pow``, ``a_div``, ``coefficients``, ``exponents``, stored through the inverse softplus) and the buffer
    ``ke`` are the reference's, so its ``state_dict``s and pickles load.

    In eval mode, on float32 device tensors and with ``cutoff_fn`` None or the mirror ``CosineCutoff``, the energy is ONE operator,
    ``torch.ops.spk_hip.zbl`` (csrc/spk_zbl.hip), whose backward returns dE/dr_ij -- what ``Forces`` asks for.  Everything else runs
    the reference's formula on ATen, on whatever device the tensors are on: training mode (gradients w.r.t. the four parameters and
    the second order ``Forces(create_graph=True)`` needs), host tensors, float64, any other cutoff callable.  Gradients w.r.t. the
    parameters from the HIP operator are deliberately not provided: a trainable ZBL term trains on the ATen route.

    The operator reads the effective parameters (after softplus / L1 normalisation) from a 12-float device buffer.  ``op_params()`` --
    host code, run by every eager call of the module or of the fused model route -- rewrites that buffer IN PLACE when a parameter, ``ke``
    or the radius has changed, so a captured HIP graph, which keeps pointing at the buffer, replays with the new values after ONE such
    eager call; a bare ``graph.replay()`` straight after a parameter update still reads the old ones.  Moving the module to another device
    makes a new buffer: capture again.  Under TorchScript the 12 floats are computed in every call, with the cutoff radius the module had
    when it was scripted (``load_state_dict`` before scripting is seen; a change of ``cutoff_fn.cutoff`` afterwards is not)."""

    _zbl_op: Final[bool]

    def __init__(self, energy_unit: Union[str, float], position_unit: Union[str, float], output_key: str, trainable: bool = True,
                 cutoff_fn: Optional[Callable] = None, n_molecules_key: str = "_n_molecules"):
        super().__init__()
        energy_units = spk_units.convert_units("Ha", energy_unit)
        position_units = spk_units.convert_units("Bohr", position_unit)
        ke = energy_units * position_units
        self.register_buffer("ke", torch.tensor(ke))
        self.cutoff_fn = cutoff_fn
        self.output_key = output_key
        # all quantities have a fixed sign: stored as the inverse softplus, a softplus in forward() restores them
        a_div = _softplus_inverse(torch.tensor([1.0 / (position_units * 0.8854)]))      # distances can then be used directly
        a_pow = _softplus_inverse(torch.tensor([0.23]))
        exponents = _softplus_inverse(torch.tensor([3.19980, 0.94229, 0.40290, 0.20162]))
        coefficients = _softplus_inverse(torch.tensor([0.18175, 0.50986, 0.28022, 0.02817]))
        self.a_pow = nn.Parameter(a_pow, requires_grad=trainable)
        self.a_div = nn.Parameter(a_div, requires_grad=trainable)
        self.coefficients = nn.Parameter(coefficients, requires_grad=trainable)
        self.exponents = nn.Parameter(exponents, requires_grad=trainable)
        self.n_molecules_key = n_molecules_key
        self._init_operator()

    def _init_operator(self):
        self._zbl_op = self.cutoff_fn is None or type(self.cutoff_fn) is CosineCutoff
        self._zbl_rc = float(self.cutoff_fn.cutoff_value()) if type(self.cutoff_fn) is CosineCutoff else 0.0
        self.register_buffer("_zbl_params", torch.zeros(12), persistent=False)
        self._zbl_key = None

    def __setstate__(self, state):
        # a pickle made by the REFERENCE class (torch.save(model)) unpickled onto this one after install() never ran __init__
        super().__setstate__(state)
        if "n_molecules_key" not in self.__dict__:
            self.n_molecules_key = "_n_molecules"
        if "_zbl_op" not in self.__dict__ or "_zbl_params" not in self._buffers:
            self._init_operator()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        rc = state_dict.get(prefix + "cutoff_fn.cutoff")          # (children load after this module: read the radius the scripted path uses here)
        if rc is not None and type(self.cutoff_fn) is CosineCutoff and not rc.is_meta:
            self._zbl_rc = float(rc.reshape(-1)[0])

    def cutoff_radius(self) -> float:
        """Radius of the term's own cosine cutoff; 0.0 without a cutoff function."""
        return self._zbl_rc

    def _params12(self, like: torch.Tensor) -> torch.Tensor:
        """ke, cutoff (0: none), p, s, alpha[4], c[4] -- the effective values, float32 on the device of ``like``."""
        c = F.normalize(F.softplus(self.coefficients)[None, :], p=1.0, dim=1)[0]
        ke = self.ke.reshape(1).to(self.a_pow.dtype)
        rc = torch.zeros_like(self.a_pow) + self._zbl_rc
        prm = torch.cat([ke, rc, F.softplus(self.a_pow), F.softplus(self.a_div), F.softplus(self.exponents), c])
        return prm.detach().to(device=like.device, dtype=torch.float32)

    @torch.jit.unused
    def op_params(self, like: torch.Tensor) -> torch.Tensor:
        """The operator's parameter buffer, recomputed (in place: captured graphs keep pointing at it) only when a parameter, ``ke`` or the
        cutoff radius has changed since the last call."""
        if type(self.cutoff_fn) is CosineCutoff:
            self._zbl_rc = float(self.cutoff_fn.cutoff_value())
        ps = (self.ke, self.a_pow, self.a_div, self.exponents, self.coefficients)
        key = (self._zbl_rc, str(like.device)) + tuple((t.data_ptr(), t._version) for t in ps)
        if key != self._zbl_key or self._zbl_params.device != like.device:
            with torch.no_grad():
                prm = self._params12(like)
                if self._zbl_params.device != like.device or self._zbl_params.dtype != torch.float32:
                    self._zbl_params = prm.clone()
                else:
                    self._zbl_params.copy_(prm)
            self._zbl_key = key
        return self._zbl_params

    def _n_molecules(self, inputs: Dict[str, torch.Tensor], idx_m: torch.Tensor) -> int:
        # like Atomwise: a host-side molecule count in the batch avoids the reference's int(idx_m[-1]) + 1 (a device sync)
        if self.n_molecules_key in inputs:
            return int(inputs[self.n_molecules_key])
        return int(idx_m[-1]) + 1

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        z = inputs[properties.Z]
        r_ij = inputs[properties.Rij]
        idx_i = inputs[properties.idx_i]
        idx_j = inputs[properties.idx_j]
        idx_m = inputs[properties.idx_m]
        n_molecules = self._n_molecules(inputs, idx_m)
        if self._zbl_op and not self.training and not use_aten(r_ij):
            if torch.jit.is_scripting():
                prm = self._params12(r_ij)
            else:
                prm = self.op_params(r_ij)
            inputs[self.output_key] = torch.ops.spk_hip.zbl(r_ij, z, idx_i, idx_j, idx_m, n_molecules, prm)[0]
            return inputs
        if use_aten(r_ij):
            note_fallback()
        # the reference's formula (atomistic/nuclear_repulsion.py:70-106), differentiable to any order in positions and parameters
        d_ij = torch.norm(r_ij, dim=1)
        n_atoms = z.shape[0]
        a = z ** F.softplus(self.a_pow)
        a_ij = (a[idx_i] + a[idx_j]) * F.softplus(self.a_div)
        exponents = a_ij[..., None] * F.softplus(self.exponents)[None, ...]
        coefficients = F.softplus(self.coefficients)[None, ...]
        coefficients = F.normalize(coefficients, p=1.0, dim=1)
        screening = torch.sum(coefficients * torch.exp(-exponents * d_ij[:, None]), dim=1)
        repulsion = (z[idx_i] * z[idx_j]) / d_ij
        if self.cutoff_fn is not None:
            f_cut = self.cutoff_fn(d_ij)
            repulsion = repulsion * f_cut
        y_zbl = scatter_add(repulsion * screening, idx_i, dim_size=n_atoms)
        y_zbl = scatter_add(y_zbl, idx_m, dim_size=n_molecules)
        y_zbl = 0.5 * self.ke * y_zbl
        inputs[self.output_key] = y_zbl
        return inputs


class Aggregation(nn.Module):
    """Sum of several predictions under one key (atomistic/aggregation.py:9-28), e.g. learned energy + ZBL repulsion -> ``energy``."""

    def __init__(self, keys: List[str], output_key: str = "y"):
        super().__init__()
        self.keys: List[str] = list(keys)
        self.output_key = output_key
        self.model_outputs = [output_key]

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        energy = torch.stack([inputs[key] for key in self.keys]).sum(0)
        inputs[self.output_key] = energy
        return inputs
