"""Mirrors of the reference *callers* either side of the hot path, so that a complete force call can be
assembled (and scripted) without the reference package: ``Strain`` (atomistic/response.py:434-464), ``PairwiseDistances``
(atomistic/distances.py:9-26), ``Atomwise`` (atomistic/atomwise.py:14-88) and ``Forces`` (atomistic/response.py:18-92).  In an integration the
reference's own modules run unchanged on top of the HIP classes (tests/test_gpu_reference_callers.py) -- they only see
``schnetpack.nn.scatter_add`` / ``Dense`` / the representation classes; ``install(fused_head=True)`` swaps in this
``Atomwise`` for its one-kernel energy head.  ``ZBLRepulsionEnergy`` (atomistic/nuclear_repulsion.py:13-108) and ``Aggregation``
(atomistic/aggregation.py:9-28) add the short-range nuclear repulsion production potentials carry next to the learned energy.
``DipoleMoment`` and ``Polarizability`` (atomistic/atomwise.py:91-293) are the tensorial heads on PaiNN's vector representation.
``FilterShortRange`` (atomistic/distances.py:29-57), ``CoulombPotential``, ``DampedCoulombPotential``, ``EnergyCoulomb`` and ``EnergyEwald``
(atomistic/electrostatic.py) are the point-charge electrostatics that consume the partial charges.
"""
import math
from typing import Callable, Dict, Final, List, Optional, Sequence, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, properties
from . import units as spk_units
from . import torchops  # noqa: F401  (registers torch.ops.spk_hip)
from .nn import CosineCutoff, Dense, GatedEquivariantBlock, SwitchFunction, build_gated_equivariant_mlp, build_mlp, scatter_add
from .nn.base import activation_id
from .nn.fallback import note_fallback, use_aten

__all__ = ["Strain", "PairwiseDistances", "Atomwise", "Forces", "ZBLRepulsionEnergy", "Aggregation", "DipoleMoment", "Polarizability",
           "FilterShortRange", "CoulombPotential", "DampedCoulombPotential", "EnergyCoulomb", "EnergyEwald", "EnergyEwaldError"]


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


def _gated_head_act(net, n_in: int) -> int:
    """Activation id (> 0) when ``net`` is the gated equivariant MLP the one-launch kernel covers -- ``build_gated_equivariant_mlp(n_in, 1)``
    with the pyramidal default widths, the gating networks as wide as their block's input, one fusable activation inside and on the scalars
    of every block but the last -- else 0."""
    if not (isinstance(net, nn.Sequential) and len(net) >= 1 and all(type(b) is GatedEquivariantBlock for b in net)):
        return 0
    act0 = activation_id(net[0].scalar_net[0].activation)
    if act0 is None or act0 == _lib.SPK_ACT_NONE:
        return 0
    n = int(n_in)
    for i, b in enumerate(net):
        last = i == len(net) - 1
        m = 1 if last else n // 2
        if (b.n_sin, b.n_vin, b.n_sout, b.n_vout, b.n_hidden) != (n, n, m, m, n):
            return 0
        sn = b.scalar_net
        if not (type(b.mix_vectors) is Dense and b.mix_vectors.bias is None and len(sn) == 2 and all(type(l) is Dense for l in sn)):
            return 0
        if sn[0].bias is None or sn[1].bias is None or activation_id(sn[0].activation) != act0 or activation_id(sn[1].activation) != _lib.SPK_ACT_NONE:
            return 0
        sact = _lib.SPK_ACT_NONE if b.sactivation is None else activation_id(b.sactivation)
        if sact != (_lib.SPK_ACT_NONE if last else act0):
            return 0
        n = m
    if not bool(_lib.lib().spk_gated_mlp_supported(int(n_in), len(net), int(act0))):
        return 0
    return int(act0)


def _scalar_head_act(net) -> int:
    """Activation id (> 0) when ``net`` is the 2-layer / width-1 ``build_mlp`` head that ``spk_atomwise_fwd_f32`` covers, else 0."""
    if not (isinstance(net, nn.Sequential) and len(net) == 2 and all(type(l) is Dense for l in net)):
        return 0
    act = activation_id(net[0].activation)
    if act is None or act == _lib.SPK_ACT_NONE or activation_id(net[1].activation) != _lib.SPK_ACT_NONE:
        return 0
    if net[1].out_features != 1 or net[0].bias is None or net[1].bias is None:
        return 0
    if not bool(_lib.lib().spk_atomwise_supported(int(net[0].in_features), int(net[0].out_features), int(act))):
        return 0
    return int(act)


class DipoleMoment(nn.Module):
    """Dipole moment from latent partial charges and, with ``use_vector_representation``, local atomic dipoles (atomistic/atomwise.py:91-213):
    ``mu = sum_i q_i R_i + d_i``; ``correct_charges`` shifts the charges of every molecule so that they sum to ``inputs["total_charge"]`` (zero when
    absent).  Constructor, attributes and ``state_dict`` keys are the reference's.

    Eval mode on float32 device tensors is two launches: the whole gated equivariant MLP (``torch.ops.spk_hip.gated_mlp``; scalar route: the
    ``atomwise`` operator's per-atom output) and the per-molecule part (``torch.ops.spk_hip.dipole_moment``: charge sum, correction, moment; no float
    atomics, ``idx_m`` ascending).  No autograd graph is built there: with autograd enabled the outputs pass through ``eval_guard``, whose backward
    raises.  Training mode, float64, host tensors and heads without a fused kernel (any ``n_hidden`` / ``n_layers`` but the default two pyramidal
    layers of width 64 or 128, other activations) run the reference's formula on the ``Dense`` / ``scatter_add`` mirrors -- the route with parameter
    gradients and derivatives w.r.t. the positions.  A molecule without atoms gets a zero moment on both routes (the reference's 0 / 0 correction of
    such a molecule is never gathered by an atom).  ``_n_atoms`` is read on the ATen route only, and counted from ``idx_m`` when absent.

    When a later ``EnergyCoulomb`` / ``EnergyEwald`` of the model reads ``charges_key``, ``NeuralNetworkPotential`` sets ``_charges_differentiable``: with
    autograd enabled the head then runs that differentiable route in eval mode as well (no ``eval_guard``), so ``Forces`` of the electrostatic energy
    includes the dq/dR term; under ``torch.no_grad()`` it keeps the two fused launches."""

    use_vector_representation: Final[bool]
    _gated_act: Final[int]
    _scalar_act: Final[int]
    #: set by ``NeuralNetworkPotential`` (and by ``install()``'s hook on the reference's model) when a later ``EnergyCoulomb`` / ``EnergyEwald`` reads
    #: ``charges_key``: with autograd enabled the head then runs its differentiable ``outnet`` route in eval mode too, so that ``Forces`` of the
    #: electrostatic energy gets the dq/dR term.  False (the default): the two fused launches, outputs behind ``eval_guard``.
    _charges_differentiable: bool

    def __init__(self, n_in: int, n_hidden: Optional[Union[int, Sequence[int]]] = None, n_layers: int = 2, activation: Callable = F.silu,
                 predict_magnitude: bool = False, return_charges: bool = False, dipole_key: str = properties.dipole_moment,
                 charges_key: str = properties.partial_charges, correct_charges: bool = True, use_vector_representation: bool = False,
                 n_molecules_key: str = "_n_molecules"):
        super().__init__()
        self.dipole_key = dipole_key
        self.charges_key = charges_key
        self.return_charges = return_charges
        self.model_outputs = [dipole_key]
        if self.return_charges:
            self.model_outputs.append(charges_key)
        self.predict_magnitude = predict_magnitude
        self.use_vector_representation = use_vector_representation
        self.correct_charges = correct_charges
        if use_vector_representation:
            self.outnet = build_gated_equivariant_mlp(n_in=n_in, n_out=1, n_hidden=n_hidden, n_layers=n_layers, activation=activation,
                                                      sactivation=activation)
        else:
            self.outnet = build_mlp(n_in=n_in, n_out=1, n_hidden=n_hidden, n_layers=n_layers, activation=activation)
        self.n_molecules_key = n_molecules_key
        self._charges_differentiable = False
        self._init_operator()

    def _init_operator(self):
        self._gated_act = _gated_head_act(self.outnet, self.outnet[0].n_sin) if self.use_vector_representation else 0
        self._scalar_act = 0 if self.use_vector_representation else _scalar_head_act(self.outnet)

    def __setstate__(self, state):
        # a pickle made by the REFERENCE class unpickled onto this one after install() never ran __init__
        super().__setstate__(state)
        if "n_molecules_key" not in self.__dict__:
            self.n_molecules_key = "_n_molecules"
        if "_gated_act" not in self.__dict__ or "_scalar_act" not in self.__dict__:
            self._init_operator()
        if "_charges_differentiable" not in self.__dict__:
            self._charges_differentiable = False

    def _n_molecules(self, inputs: Dict[str, torch.Tensor], idx_m: torch.Tensor) -> int:
        # like Atomwise: a host-side molecule count in the batch avoids the reference's int(idx_m[-1]) + 1 (a device sync)
        if self.n_molecules_key in inputs:
            return int(inputs[self.n_molecules_key])
        return int(idx_m[-1]) + 1

    def _head_weights(self) -> List[torch.Tensor]:
        ws: List[torch.Tensor] = []
        for b in self.outnet:
            ws.append(b.mix_vectors.weight)
            ws.append(b.scalar_net[0].weight)
            ws.append(b.scalar_net[0].bias)
            ws.append(b.scalar_net[1].weight)
            ws.append(b.scalar_net[1].bias)
        return ws

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        positions = inputs[properties.R]
        l0 = inputs["scalar_representation"]
        idx_m = inputs[properties.idx_m]
        maxm = self._n_molecules(inputs, idx_m)
        total: Optional[torch.Tensor] = None
        if properties.total_charge in inputs:
            total = inputs[properties.total_charge]
        device_ok = not self.training and l0.dim() == 2 and not use_aten(l0) and not use_aten(positions)
        if self._charges_differentiable and torch.is_grad_enabled():      # an electrostatic term differentiates the charges it reads
            device_ok = False
        if self.use_vector_representation:
            l1 = inputs["vector_representation"]
            if self._gated_act > 0 and device_ok and l1.dim() == 3:
                q, d = torch.ops.spk_hip.gated_mlp(l0.detach(), l1.detach(), self._head_weights(), self._gated_act)
                return self._moment(inputs, q, d, positions, idx_m, maxm, total, self.outnet[0].mix_vectors.weight)
            charges, dip = self.outnet((l0, l1))
            return self._aten(inputs, charges, torch.squeeze(dip, -1), positions, idx_m, maxm, total)
        else:
            if self._scalar_act > 0 and device_ok:
                n0 = self.outnet[0]
                n1 = self.outnet[1]
                q = torch.ops.spk_hip.atomwise(l0.detach(), n0.weight.detach(), n0.bias.detach(), n1.weight.detach(), n1.bias.detach(), idx_m, maxm,
                                               self._scalar_act)[1]
                return self._moment(inputs, q, None, positions, idx_m, maxm, total, n0.weight)
            charges = self.outnet(l0)
            return self._aten(inputs, charges, None, positions, idx_m, maxm, total)

    def _moment(self, inputs: Dict[str, torch.Tensor], q: torch.Tensor, d: Optional[torch.Tensor], positions: torch.Tensor, idx_m: torch.Tensor,
                maxm: int, total: Optional[torch.Tensor], guard: torch.Tensor) -> Dict[str, torch.Tensor]:
        y, charges = torch.ops.spk_hip.dipole_moment(q, d, positions.detach(), idx_m, maxm, total, self.correct_charges)
        if self.predict_magnitude:
            y = torch.norm(y, dim=1, keepdim=False)
        if torch.is_grad_enabled():      # a backward pass into the eval-mode head gets the eval-only message, not silence
            y = torch.ops.spk_hip.eval_guard(y, [guard])
            charges = torch.ops.spk_hip.eval_guard(charges, [guard])
        if self.return_charges:
            inputs[self.charges_key] = charges
        inputs[self.dipole_key] = y
        return inputs

    def _aten(self, inputs: Dict[str, torch.Tensor], charges: torch.Tensor, dip: Optional[torch.Tensor], positions: torch.Tensor,
              idx_m: torch.Tensor, maxm: int, total: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
        # the reference's formula (atomistic/atomwise.py:187-212)
        if use_aten(charges):
            note_fallback()
        if self.correct_charges:
            sum_charge = scatter_add(charges, idx_m, dim_size=maxm)
            if total is not None:
                total_charge = total[:, None]
            else:
                total_charge = torch.zeros_like(sum_charge)
            if properties.n_atoms in inputs:
                natoms = inputs[properties.n_atoms].to(charges.dtype).unsqueeze(-1)
            else:
                natoms = scatter_add(torch.ones_like(charges), idx_m, dim_size=maxm)
            charge_correction = (total_charge - sum_charge) / natoms
            charge_correction = charge_correction[idx_m]
            charges = charges + charge_correction
        if self.return_charges:
            inputs[self.charges_key] = charges
        y = positions * charges
        if dip is not None:
            y = y + dip
        y = scatter_add(y, idx_m, dim_size=maxm)
        if self.predict_magnitude:
            y = torch.norm(y, dim=1, keepdim=False)
        inputs[self.dipole_key] = y
        return inputs


class Polarizability(nn.Module):
    """Polarizability tensor by rank factorisation (atomistic/atomwise.py:216-293): ``alpha = sum_i a_i 1 + d_i R_i^T + R_i d_i^T`` with the scalar
    ``a_i`` and the vector ``d_i`` from a gated equivariant MLP on the scalar and vector representation.  Constructor, attributes and
    ``state_dict`` keys are the reference's.

    Routing as :class:`DipoleMoment`: eval mode on float32 device tensors is ``torch.ops.spk_hip.gated_mlp`` +
    ``torch.ops.spk_hip.polarizability`` (two launches; ``alpha`` equals its transpose to the bit; ``idx_m`` ascending), everything else the
    reference's formula on the mirrors."""

    _gated_act: Final[int]

    def __init__(self, n_in: int, n_hidden: Optional[Union[int, Sequence[int]]] = None, n_layers: int = 2, activation: Callable = F.silu,
                 polarizability_key: str = properties.polarizability, n_molecules_key: str = "_n_molecules"):
        super().__init__()
        self.n_in = n_in
        self.n_layers = n_layers
        self.n_hidden = n_hidden
        self.polarizability_key = polarizability_key
        self.model_outputs = [polarizability_key]
        self.outnet = build_gated_equivariant_mlp(n_in=n_in, n_out=1, n_hidden=n_hidden, n_layers=n_layers, activation=activation,
                                                  sactivation=activation)
        self.requires_dr = False
        self.requires_stress = False
        self.n_molecules_key = n_molecules_key
        self._gated_act = _gated_head_act(self.outnet, n_in)

    def __setstate__(self, state):
        super().__setstate__(state)
        if "n_molecules_key" not in self.__dict__:
            self.n_molecules_key = "_n_molecules"
        if "_gated_act" not in self.__dict__:
            self._gated_act = _gated_head_act(self.outnet, self.outnet[0].n_sin)

    def _n_molecules(self, inputs: Dict[str, torch.Tensor], idx_m: torch.Tensor) -> int:
        if self.n_molecules_key in inputs:
            return int(inputs[self.n_molecules_key])
        return int(idx_m[-1]) + 1

    def _head_weights(self) -> List[torch.Tensor]:
        ws: List[torch.Tensor] = []
        for b in self.outnet:
            ws.append(b.mix_vectors.weight)
            ws.append(b.scalar_net[0].weight)
            ws.append(b.scalar_net[0].bias)
            ws.append(b.scalar_net[1].weight)
            ws.append(b.scalar_net[1].bias)
        return ws

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        positions = inputs[properties.R]
        l0 = inputs["scalar_representation"]
        l1 = inputs["vector_representation"]
        idx_m = inputs[properties.idx_m]
        maxm = self._n_molecules(inputs, idx_m)
        if (self._gated_act > 0 and not self.training and l0.dim() == 2 and l1.dim() == 3 and l1.shape[-2] == 3 and not use_aten(l0)
                and not use_aten(positions)):
            a0, d = torch.ops.spk_hip.gated_mlp(l0.detach(), l1.detach(), self._head_weights(), self._gated_act)
            alpha = torch.ops.spk_hip.polarizability(a0, d, positions.detach(), idx_m, maxm)
            if torch.is_grad_enabled():
                alpha = torch.ops.spk_hip.eval_guard(alpha, [self.outnet[0].mix_vectors.weight])
            inputs[self.polarizability_key] = alpha
            return inputs
        if use_aten(l0):
            note_fallback()
        # the reference's formula (atomistic/atomwise.py:267-292)
        dim = l1.shape[-2]
        l0, l1 = self.outnet((l0, l1))
        alpha = l0[..., 0:1]
        size = list(alpha.shape)
        size[-1] = dim
        alpha = alpha.expand(size)
        alpha = torch.diag_embed(alpha)
        mur = l1[..., None, 0] * positions[..., None, :]
        alpha_c = mur + mur.transpose(-2, -1)
        alpha = alpha + alpha_c
        alpha = scatter_add(alpha, idx_m, dim_size=maxm)
        inputs[self.polarizability_key] = alpha
        return inputs


class FilterShortRange(nn.Module):
    """Separate the short-range pairs from all supplied pairs (atomistic/distances.py:29-57): the full list moves to the long-range keys
    (``_Rij_lr``, ``_idx_i_lr``, ``_idx_j_lr``) and the pairs with ``d <= short_range_cutoff`` stay under the original keys.  The reference's formula
    on ATen (a compaction with a data-dependent size: plumbing, not a hot path)."""

    def __init__(self, short_range_cutoff: float):
        super().__init__()
        self.short_range_cutoff = short_range_cutoff

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        idx_i = inputs[properties.idx_i]
        idx_j = inputs[properties.idx_j]
        Rij = inputs[properties.Rij]
        rij = torch.norm(Rij, dim=-1)
        cidx = torch.nonzero(rij <= self.short_range_cutoff).squeeze(-1)
        inputs[properties.Rij_lr] = Rij
        inputs[properties.idx_i_lr] = idx_i
        inputs[properties.idx_j_lr] = idx_j
        inputs[properties.Rij] = Rij[cidx]
        inputs[properties.idx_i] = idx_i[cidx]
        inputs[properties.idx_j] = idx_j[cidx]
        return inputs


class CoulombPotential(nn.Module):
    """1 / d (atomistic/electrostatic.py:14-23)."""

    def forward(self, d_ij: torch.Tensor) -> torch.Tensor:
        return 1.0 / d_ij


class DampedCoulombPotential(nn.Module):
    """PhysNet's damped Coulomb potential ``s(d) / sqrt(d^2 + 1) + (1 - s(d)) / d`` (atomistic/electrostatic.py:26-57)."""

    def __init__(self, switch_fn: nn.Module):
        super().__init__()
        self.switch_fn = switch_fn

    def forward(self, d_ij: torch.Tensor) -> torch.Tensor:
        potential = 1.0 / d_ij
        damped = 1.0 / torch.sqrt(d_ij ** 2 + 1)
        f_switch = self.switch_fn(d_ij)
        return f_switch * damped + (1 - f_switch) * potential


class EnergyEwaldError(Exception):
    pass


def _pair_kind(potential) -> int:
    """Pair function of csrc/spk_coulomb.hip for a potential module: 0 the mirror ``CoulombPotential``, 1 the mirror ``DampedCoulombPotential``
    around the mirror ``SwitchFunction``, -1 anything else (ATen route)."""
    if type(potential) is CoulombPotential:
        return 0
    if type(potential) is DampedCoulombPotential and type(potential.switch_fn) is SwitchFunction:
        return 1
    return -1


class EnergyCoulomb(nn.Module):
    """Coulomb energy of point charges by direct summation over a neighbour list (atomistic/electrostatic.py:60-152):
    ``E = 1/2 ke sum_pairs q_i q_j chi(d_ij)``; with ``cutoff`` the potential is shifted (``chi + shift^2 / chi - 2 shift`` for ``d <= cutoff``, zero
    beyond) so that it and its slope vanish at the cutoff.  Constructor, attributes and buffers (``ke`` [1], 0-dim ``cutoff`` and ``shift``) are
    the reference's, so its ``state_dict``s and pickles load.

    In eval mode, on float32 device tensors and with ``coulomb_potential`` the mirror ``CoulombPotential`` or the mirror ``DampedCoulombPotential``
    around the mirror ``SwitchFunction``, the energy is ONE operator, ``torch.ops.spk_hip.coulomb`` (csrc/spk_coulomb.hip), whose backward returns
    dE/dr_ij and dE/dq -- what ``Forces`` asks for, also through predicted charges.  Everything else runs the reference's formula on ATen, on
    whatever device the tensors are on (``note_fallback()``): training mode (second order for ``Forces(create_graph=True)``), float64, host tensors,
    any other potential callable.

    The operator reads 8 floats from a device buffer that ``op_params()`` -- host code, run by every eager call -- rewrites IN PLACE when ``ke``,
    ``cutoff``, ``shift`` or the switch radii have changed, so a captured HIP graph replays with the new values after one eager call.  Under
    TorchScript the floats are those the module had when it was scripted.  A host-side molecule count under ``_n_molecules`` in the batch avoids
    the reference's ``int(idx_m[-1]) + 1`` (a device sync)."""

    _kind: Final[int]
    use_neighbors_lr: Final[bool]

    def __init__(self, energy_unit: Union[str, float], position_unit: Union[str, float], coulomb_potential: nn.Module, output_key: str,
                 charges_key: str = properties.partial_charges, use_neighbors_lr: bool = True, cutoff: Optional[float] = None,
                 n_molecules_key: str = "_n_molecules"):
        super().__init__()
        ke = spk_units.convert_units("Ha", energy_unit) * spk_units.convert_units("Bohr", position_unit)
        self.register_buffer("ke", torch.Tensor([ke]))
        self.coulomb_potential = coulomb_potential
        self.charges_key = charges_key
        self.output_key = output_key
        self.model_outputs = [output_key]
        self.use_neighbors_lr = use_neighbors_lr
        if cutoff is not None:
            cutoff = torch.tensor(cutoff)
            shift = self.coulomb_potential(cutoff).detach()
            self.register_buffer("cutoff", cutoff)
            self.register_buffer("shift", shift)
        else:
            self.cutoff = None
            self.shift = None
        self.n_molecules_key = n_molecules_key
        self._init_operator()

    def _init_operator(self):
        self._kind = _pair_kind(self.coulomb_potential)
        self.register_buffer("_op_params", torch.zeros(8), persistent=False)
        self._op_key = None
        self._read_host()

    def _read_host(self):
        """Host copies of the buffers (read when they change, not per call)."""
        self._ke_host = float(self.ke.reshape(-1)[0])
        self._rc_host = float(self.cutoff) if self.cutoff is not None else 0.0
        self._shift_host = float(self.shift) if self.shift is not None else 0.0
        self._on_host, self._off_host = 0.0, 1.0
        if self._kind == 1:
            self._on_host, self._off_host = self.coulomb_potential.switch_fn.switch_values()

    def __setstate__(self, state):
        # a pickle made by the REFERENCE class unpickled onto this one after install() never ran __init__
        super().__setstate__(state)
        if "n_molecules_key" not in self.__dict__:
            self.n_molecules_key = "_n_molecules"
        if "_kind" not in self.__dict__ or "_op_params" not in self._buffers:
            self._init_operator()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if not self.ke.is_meta:
            self._read_host()
            on = state_dict.get(prefix + "coulomb_potential.switch_fn.switch_on")      # (children load after this module)
            off = state_dict.get(prefix + "coulomb_potential.switch_fn.switch_off")
            if self._kind == 1 and on is not None and off is not None and not on.is_meta:
                self._on_host, self._off_host = float(on.reshape(-1)[0]), float(off.reshape(-1)[0])
            self._op_key = None

    def _params8(self, like: torch.Tensor) -> torch.Tensor:
        """ke, kind, cutoff (0: none), shift, switch_on, switch_off, 0, 0 as float32 on the device of ``like``."""
        return torch.tensor([self._ke_host, float(self._kind), self._rc_host, self._shift_host, self._on_host, self._off_host, 0.0, 0.0],
                            dtype=torch.float32, device=like.device)

    @torch.jit.unused
    def op_params(self, like: torch.Tensor) -> torch.Tensor:
        """The operator's parameter buffer, rewritten (in place: captured graphs keep pointing at it) only when a buffer or a switch radius has
        changed since the last call."""
        bufs = [self.ke] + ([self.cutoff, self.shift] if self.cutoff is not None else [])
        sw = self.coulomb_potential.switch_fn.switch_values() if self._kind == 1 else (0.0, 1.0)
        key = (str(like.device), sw) + tuple((t.data_ptr(), t._version) for t in bufs)
        if key != self._op_key or self._op_params.device != like.device:
            self._read_host()
            with torch.no_grad():
                prm = self._params8(like)
                if self._op_params.device != like.device or self._op_params.dtype != torch.float32:
                    self._op_params = prm
                else:
                    self._op_params.copy_(prm)
            self._op_key = key
        return self._op_params

    def _n_molecules(self, inputs: Dict[str, torch.Tensor], idx_m: torch.Tensor) -> int:
        if self.n_molecules_key in inputs:
            return int(inputs[self.n_molecules_key])
        return int(idx_m[-1]) + 1

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        q = inputs[self.charges_key].squeeze(-1)
        idx_m = inputs[properties.idx_m]
        if self.use_neighbors_lr:
            r_ij = inputs[properties.Rij_lr]
            idx_i = inputs[properties.idx_i_lr]
            idx_j = inputs[properties.idx_j_lr]
        else:
            r_ij = inputs[properties.Rij]
            idx_i = inputs[properties.idx_i]
            idx_j = inputs[properties.idx_j]
        n_molecules = self._n_molecules(inputs, idx_m)
        if self._kind >= 0 and not self.training and not use_aten(r_ij) and not use_aten(q):
            if torch.jit.is_scripting():
                prm = self._params8(r_ij)
            else:
                prm = self.op_params(r_ij)
            inputs[self.output_key] = torch.ops.spk_hip.coulomb(r_ij, q, idx_i, idx_j, idx_m, n_molecules, prm)[0]
            return inputs
        note_fallback()
        # the reference's formula (atomistic/electrostatic.py:131-151), differentiable to any order
        d_ij = torch.norm(r_ij, dim=1)
        n_atoms = q.shape[0]
        q_ij = q[idx_i] * q[idx_j]
        potential = self.coulomb_potential(d_ij)
        cutoff = self.cutoff
        shift = self.shift
        if cutoff is not None and shift is not None:
            potential = potential + shift ** 2 / potential - 2.0 * shift
            potential = torch.where(d_ij <= cutoff, potential, torch.zeros_like(potential))
        y = scatter_add((q_ij * potential), idx_i, dim_size=n_atoms)
        y = scatter_add(y, idx_m, dim_size=n_molecules)
        y = 0.5 * self.ke * torch.squeeze(y, -1)
        inputs[self.output_key] = y
        return inputs


class EnergyEwald(nn.Module):
    """Coulomb energy of point charges in a periodic box by Ewald summation (atomistic/electrostatic.py:159-375): a real-space sum of
    ``erfc(sqrt(alpha) d) / d`` over the neighbour list (optionally screened by ``1 - screening_fn(d)``) plus the reciprocal-space sum over the
    integer vectors ``kvecs`` and the self-interaction term.  Constructor, attributes and buffers (``ke`` [1], ``alpha`` [1], ``kvecs`` [K, 3], in the
    reference's order) are the reference's, so its ``state_dict``s and pickles load.

    In eval mode, on float32 device tensors, with ``screening_fn`` None or the mirror ``SwitchFunction``, ``k_max <= 8`` (the factor table of
    csrc/spk_ewald.hip) and a cell that does not require grad, the energy is two operators: ``torch.ops.spk_hip.coulomb`` (pair function 2) and
    ``torch.ops.spk_hip.ewald_recip``, whose backwards return dE/dr_ij, dE/dR and dE/dq.  Everything else runs the reference's formula on ATen
    (``note_fallback()``): training mode, float64, host tensors, another screening callable, ``k_max`` beyond the cap, and a strained cell -- the
    route of the Ewald stress.  A cell without volume raises ``EnergyEwaldError`` on the ATen route like the reference; on the operator route it
    yields NaN for that molecule (raising would need a device sync).  Parameters reach the kernels as in :class:`EnergyCoulomb`."""

    _screen: Final[int]
    use_neighbors_lr: Final[bool]
    k_max: Final[int]

    def __init__(self, alpha: float, k_max: int, energy_unit: Union[str, float], position_unit: Union[str, float], output_key: str,
                 charges_key: str = properties.partial_charges, use_neighbors_lr: bool = True, screening_fn: Optional[nn.Module] = None,
                 n_molecules_key: str = "_n_molecules"):
        super().__init__()
        ke = spk_units.convert_units("Ha", energy_unit) * spk_units.convert_units("Bohr", position_unit)
        self.register_buffer("ke", torch.Tensor([ke]))
        self.charges_key = charges_key
        self.output_key = output_key
        self.model_outputs = [output_key]
        self.use_neighbors_lr = use_neighbors_lr
        self.screening_fn = screening_fn
        self.register_buffer("alpha", torch.Tensor([alpha]))
        self.k_max = k_max
        kvecs = self._generate_kvecs()
        self.register_buffer("kvecs", kvecs)
        self.n_molecules_key = n_molecules_key
        self._init_operator()

    @torch.jit.unused
    def _generate_kvecs(self) -> torch.Tensor:
        """The integer k-vectors, in the reference's order (atomistic/electrostatic.py:209-224)."""
        krange = torch.arange(0, self.k_max + 1, dtype=self.alpha.dtype)
        krange = torch.cat([krange, -krange[1:]])
        kvecs = torch.cartesian_prod(krange, krange, krange)
        norm = torch.sum(kvecs ** 2, dim=1)
        kvecs = kvecs[norm <= self.k_max ** 2 + 2, :]
        norm = norm[norm <= self.k_max ** 2 + 2]
        kvecs = kvecs[norm != 0, :]
        return kvecs

    def _init_operator(self):
        self._screen = 0 if self.screening_fn is None else (1 if type(self.screening_fn) is SwitchFunction else -1)
        self._kmax_ok = 0 < int(self.k_max) <= int(_lib.lib().spk_ewald_max_kmax())
        self.register_buffer("_op_params", torch.zeros(10), persistent=False)
        self._op_key = None
        self._read_host()

    def _read_host(self):
        self._ke_host = float(self.ke.reshape(-1)[0])
        self._alpha_host = float(self.alpha.reshape(-1)[0])
        self._on_host, self._off_host = 0.0, 1.0
        if self._screen == 1:
            self._on_host, self._off_host = self.screening_fn.switch_values()

    def __setstate__(self, state):
        super().__setstate__(state)
        if "n_molecules_key" not in self.__dict__:
            self.n_molecules_key = "_n_molecules"
        if "_screen" not in self.__dict__ or "_op_params" not in self._buffers:
            self._init_operator()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if not self.ke.is_meta:
            self._read_host()
            on = state_dict.get(prefix + "screening_fn.switch_on")      # (children load after this module)
            off = state_dict.get(prefix + "screening_fn.switch_off")
            if self._screen == 1 and on is not None and off is not None and not on.is_meta:
                self._on_host, self._off_host = float(on.reshape(-1)[0]), float(off.reshape(-1)[0])
            self._op_key = None

    def _params10(self, like: torch.Tensor) -> torch.Tensor:
        """[0:8] the pair-function block of ``spk_hip::coulomb`` (kind 2), [8:10] ke and alpha for ``spk_hip::ewald_recip``."""
        return torch.tensor([self._ke_host, 2.0, 0.0, 0.0, self._on_host, self._off_host, self._alpha_host, 1.0 if self._screen == 1 else 0.0,
                             self._ke_host, self._alpha_host], dtype=torch.float32, device=like.device)

    @torch.jit.unused
    def op_params(self, like: torch.Tensor) -> torch.Tensor:
        """The operators' parameter buffer, rewritten in place only when ``ke``, ``alpha`` or a switch radius has changed since the last call."""
        sw = self.screening_fn.switch_values() if self._screen == 1 else (0.0, 1.0)
        key = (str(like.device), sw) + tuple((t.data_ptr(), t._version) for t in (self.ke, self.alpha))
        if key != self._op_key or self._op_params.device != like.device:
            self._read_host()
            with torch.no_grad():
                prm = self._params10(like)
                if self._op_params.device != like.device or self._op_params.dtype != torch.float32:
                    self._op_params = prm
                else:
                    self._op_params.copy_(prm)
            self._op_key = key
        return self._op_params

    def _n_molecules(self, inputs: Dict[str, torch.Tensor], idx_m: torch.Tensor) -> int:
        if self.n_molecules_key in inputs:
            return int(inputs[self.n_molecules_key])
        return int(idx_m[-1]) + 1

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        q = inputs[self.charges_key].squeeze(-1)
        idx_m = inputs[properties.idx_m]
        if self.use_neighbors_lr:
            r_ij = inputs[properties.Rij_lr]
            idx_i = inputs[properties.idx_i_lr]
            idx_j = inputs[properties.idx_j_lr]
        else:
            r_ij = inputs[properties.Rij]
            idx_i = inputs[properties.idx_i]
            idx_j = inputs[properties.idx_j]
        positions = inputs[properties.R]
        cell = inputs[properties.cell]
        n_molecules = self._n_molecules(inputs, idx_m)
        if (self._screen >= 0 and self._kmax_ok and not self.training and not use_aten(r_ij) and not use_aten(q) and not use_aten(positions)
                and not use_aten(cell) and not cell.requires_grad):
            if torch.jit.is_scripting():
                prm = self._params10(r_ij)
            else:
                prm = self.op_params(r_ij)
            y_real = torch.ops.spk_hip.coulomb(r_ij, q, idx_i, idx_j, idx_m, n_molecules, prm[0:8])[0]
            y_rec = torch.ops.spk_hip.ewald_recip(positions, q, cell, idx_m, n_molecules, self.kvecs.to(torch.float32), prm[8:10])[0]
            inputs[self.output_key] = y_real + y_rec
            return inputs
        note_fallback()
        d_ij = torch.norm(r_ij, dim=1)
        n_atoms = q.shape[0]
        y_real = self._real_space(q, d_ij, idx_i, idx_j, idx_m, n_atoms, n_molecules)
        y_reciprocal = self._reciprocal_space(q, positions, cell, idx_m, n_molecules)
        inputs[self.output_key] = y_real + y_reciprocal
        return inputs

    def _real_space(self, q: torch.Tensor, d_ij: torch.Tensor, idx_i: torch.Tensor, idx_j: torch.Tensor, idx_m: torch.Tensor, n_atoms: int,
                    n_molecules: int) -> torch.Tensor:
        """The reference's formula (atomistic/electrostatic.py:266-308)."""
        f_r = torch.erfc(torch.sqrt(self.alpha) * d_ij) / d_ij
        screening_fn = self.screening_fn
        if screening_fn is not None:
            f_r = f_r * (1.0 - screening_fn(d_ij))
        potential_ij = q[idx_i] * q[idx_j] * f_r
        y = scatter_add(potential_ij, idx_i, dim_size=n_atoms)
        y = scatter_add(y, idx_m, dim_size=n_molecules)
        return 0.5 * self.ke * y.squeeze(-1)

    @torch.jit.unused
    def _check_volume(self, v_box: torch.Tensor) -> None:
        if torch.any(torch.isclose(v_box, torch.zeros_like(v_box))):
            raise EnergyEwaldError("Simulation box has no volume.")

    def _reciprocal_space(self, q: torch.Tensor, positions: torch.Tensor, cell: torch.Tensor, idx_m: torch.Tensor, n_molecules: int) -> torch.Tensor:
        """The reference's formula (atomistic/electrostatic.py:310-375)."""
        recip_box = 2.0 * math.pi * torch.linalg.inv(cell).transpose(1, 2)
        v_box = torch.abs(torch.linalg.det(cell))
        if not torch.jit.is_scripting():      # (a scripted module cannot raise the class: a cell without volume gives inf / NaN there)
            self._check_volume(v_box)
        prefactor = 2.0 * math.pi / v_box
        kvecs = torch.matmul(self.kvecs[None, :, :], recip_box)
        k_squared = torch.sum(kvecs ** 2, dim=2)
        q_gauss = torch.exp(-0.25 * k_squared / self.alpha)
        kvec_dot_pos = torch.sum(kvecs[idx_m] * positions[:, None, :], dim=2)
        q_real = scatter_add((q[:, None] * torch.cos(kvec_dot_pos)), idx_m, dim_size=n_molecules)
        q_imag = scatter_add((q[:, None] * torch.sin(kvec_dot_pos)), idx_m, dim_size=n_molecules)
        q_dens = q_real ** 2 + q_imag ** 2
        y_ewald = prefactor * torch.sum(q_dens * q_gauss / k_squared, dim=1)
        self_interaction = math.sqrt(1.0 / math.pi) * torch.sqrt(self.alpha) * scatter_add(q ** 2, idx_m, dim_size=n_molecules)
        return self.ke * (y_ewald - self_interaction)
