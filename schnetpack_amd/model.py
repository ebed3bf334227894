"""Mirror of ``NeuralNetworkPotential`` (model/base.py:132-190) -- the one caller of the hot
path -- plus helpers to assemble the benchmark models and to move batches to the device."""
from typing import Dict, Final, List, Optional, Tuple

import torch
import torch.nn as nn

from . import properties
from .atomistic import (Aggregation, Atomwise, DipoleMoment, EnergyCoulomb, EnergyEwald, Forces, PairwiseDistances, Polarizability, Strain,
                        ZBLRepulsionEnergy)
from .nn import CosineCutoff, GaussianRBF, BesselRBF, NuclearEmbedding
from .representation import PaiNN, SchNet

__all__ = ["NeuralNetworkPotential", "build_model", "batch_to_inputs"]


def _is_forces(m) -> bool:
    """The mirror's ``Forces`` or the reference's own (atomistic/response.py:14-92; same attributes) -- not a subclass that may
    have changed what the module computes."""
    if type(m) is Forces:
        return True
    t = type(m)
    return (t.__name__ == "Forces" and t.__module__ == "schnetpack.atomistic.response"
            and all(hasattr(m, a) for a in ("calc_forces", "calc_stress", "energy_key", "force_key")))


def _is_strain(m) -> bool:
    """The mirror's ``Strain`` or the reference's own (atomistic/response.py:434-464), not a subclass."""
    t = type(m)
    return t is Strain or (t.__name__ == "Strain" and t.__module__ == "schnetpack.atomistic.response")


def _is_aggregation(m) -> bool:
    """The mirror's ``Aggregation`` or the reference's own (atomistic/aggregation.py:9-28), not a subclass."""
    t = type(m)
    if t is Aggregation:
        return True
    return (t.__name__ == "Aggregation" and t.__module__ == "schnetpack.atomistic.aggregation"
            and all(hasattr(m, a) for a in ("keys", "output_key")))


def zbl_layout(outs) -> Optional[Tuple[int, int, int, int]]:
    """Positions (head, zbl, aggregation, forces) in ``output_modules`` when they are: the learned ``Atomwise`` energy and ONE
    ``ZBLRepulsionEnergy`` on its operator path (either order), one ``Aggregation`` over exactly their two keys, ``Forces`` of the aggregated
    key.  None for every other composition."""
    if len(outs) != 4:
        return None
    if isinstance(outs[0], Atomwise) and type(outs[1]) is ZBLRepulsionEnergy:
        ih, iz = 0, 1
    elif type(outs[0]) is ZBLRepulsionEnergy and isinstance(outs[1], Atomwise):
        ih, iz = 1, 0
    else:
        return None
    head, zbl, agg, frc = outs[ih], outs[iz], outs[2], outs[3]
    if not (zbl._zbl_op and _is_aggregation(agg) and _is_forces(frc)):
        return None
    keys = list(agg.keys)
    if head.output_key == zbl.output_key or len(keys) != 2 or sorted(keys) != sorted([head.output_key, zbl.output_key]):
        return None
    if frc.energy_key != agg.output_key or agg.output_key in keys:
        return None
    return ih, iz, 2, 3


def tensorial_tail(outs) -> int:
    """Number of ``DipoleMoment`` / ``Polarizability`` mirror instances at the END of ``output_modules``.  They read the representation and the
    positions only, so the modules before them classify as if the tail were not there (:func:`classify_potential`) and the tail runs on the
    dict the fused route returns (:func:`run_tail`)."""
    n = 0
    while n < len(outs) and type(outs[len(outs) - 1 - n]) in (DipoleMoment, Polarizability):
        n += 1
    return n


def run_tail(model, inputs: Dict[str, torch.Tensor], n_tail: int) -> Dict[str, torch.Tensor]:
    """The last ``n_tail`` output modules on the dict of a fused force call (``scalar_representation``, ``vector_representation`` and the positions
    are in it)."""
    if n_tail > 0:
        outs = list(model.output_modules)
        for m in outs[len(outs) - n_tail:]:
            inputs = m(inputs)
    return inputs


def _is_electrostatic(m) -> bool:
    """The mirrors' ``EnergyCoulomb`` / ``EnergyEwald`` (subclasses included) or the reference's own (atomistic/electrostatic.py)."""
    if isinstance(m, (EnergyCoulomb, EnergyEwald)):
        return True
    t = type(m)
    return t.__name__ in ("EnergyCoulomb", "EnergyEwald") and t.__module__ == "schnetpack.atomistic.electrostatic"


def link_charge_consumers(model) -> int:
    """Tell every ``DipoleMoment(return_charges=True)`` mirror whose ``charges_key`` a LATER electrostatic output module reads that its charges are
    differentiated (``_charges_differentiable``): in eval mode with autograd enabled that head then takes its differentiable route, so ``Forces`` of
    the electrostatic energy includes the dq/dR term.  Heads without such a consumer are left as they are (two fused launches, outputs behind
    ``eval_guard``).  Returns the number of heads linked."""
    outs = list(model.output_modules)
    n = 0
    for i, m in enumerate(outs):
        if type(m) is DipoleMoment and m.return_charges:
            if any(_is_electrostatic(c) and getattr(c, "charges_key", None) == m.charges_key for c in outs[i + 1:]):
                m._charges_differentiable = True
                n += 1
    return n


def classify_potential(model) -> int:
    """0: module-by-module.  1: the standard potential -- ``PairwiseDistances`` -> fused ``SchNet`` -> ``Atomwise`` (default
    head, summed or averaged over the molecule) -> ``Forces`` without stress: representation + head are ONE operator.
    2: ... and the only other output is Forces' -dE/dR of a summed energy: energies AND forces from the two launches.
    3: ``Strain`` -> ``PairwiseDistances`` -> ... -> ``Forces(calc_forces=True, calc_stress=True)`` of the summed energy: energies,
    forces and the virial dE/dstrain from the same operators (``*_potential_stress``).
    4 / 5: forms 2 / 3 with a ``ZBLRepulsionEnergy`` next to the head, an ``Aggregation`` of the two energies and ``Forces`` of the sum
    (:func:`zbl_layout`): the same operators, then one ``zbl_forces`` operator (a row pass, two reductions, a row-pointer kernel) that adds the
    repulsion into their forces and virial, and one add of the two energies.
    A tail of ``DipoleMoment`` / ``Polarizability`` mirrors (:func:`tensorial_tail`) is set aside first: the rest classifies as above and the
    tail runs module by module behind the fused call; such a module anywhere else gives 0.  Any model with an ``EnergyCoulomb`` / ``EnergyEwald``
    term gives 0.
    Works on any model with the reference's ``NeuralNetworkPotential`` layout (model/base.py:132-190), i.e. also on the
    reference's own class around the HIP modules."""
    rep, ins, outs = model.representation, list(model.input_modules), list(model.output_modules)
    if any(_is_electrostatic(m) for m in outs):      # electrostatic terms run module by module: a fused force call must never drop them
        return 0
    outs = outs[:len(outs) - tensorial_tail(outs)]
    is_painn = isinstance(rep, PaiNN)
    if not (isinstance(rep, (SchNet, PaiNN)) and rep._fused and len(rep.interactions) > 0):
        return 0
    strained = len(ins) == 2 and _is_strain(ins[0]) and type(ins[1]) is PairwiseDistances
    if not ((strained or (len(ins) == 1 and type(ins[0]) is PairwiseDistances)) and len(outs) >= 1):
        return 0
    lay = zbl_layout(outs)
    if lay is not None:
        head, frc = outs[lay[0]], outs[lay[3]]
        if not (head._fused_head and head.per_atom_output_key is None and head.aggregation_mode == "sum" and frc.calc_forces):
            return 0
        if strained:
            return 5 if frc.calc_stress else 0
        return 0 if frc.calc_stress else 4
    head = outs[0]
    if not (isinstance(head, Atomwise) and head._fused_head and head.per_atom_output_key is None
            and head.aggregation_mode in ("sum", "avg")):
        return 0
    if strained:
        frc = outs[1] if len(outs) == 2 else None
        ok = (frc is not None and _is_forces(frc) and frc.calc_forces and frc.calc_stress and frc.energy_key == head.output_key
              and head.aggregation_mode == "sum")
        return 3 if ok else 0
    if not all(_is_forces(m) and not m.calc_stress for m in outs[1:]):
        return 0
    if (len(outs) == 2 and outs[1].calc_forces and outs[1].energy_key == head.output_key and head.aggregation_mode == "sum"):
        return 2
    return 0 if is_painn else 1          # (PaiNN: only the energies-and-forces form is one operator)


def potential_forward(model, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Standard potential, differentiable form: ``torch.ops.spk_hip.schnet_potential`` (pair vectors, representation and
    energy head in one launch each way); the ``Forces`` module that follows triggers the one-launch backward."""
    rep, head = model.representation, model.output_modules[0]
    idx_m = inputs[properties.idx_m]
    n_mol = head._n_molecules(inputs, idx_m)
    kind, p0, p1 = rep.radial_basis.kernel_params()
    l0, l1 = head.outnet[0], head.outnet[1]
    E, x = torch.ops.spk_hip.schnet_potential(
        rep.embed(inputs), inputs[properties.R], inputs.get(properties.offsets), inputs[properties.idx_i], inputs[properties.idx_j], idx_m,
        n_mol, rep.interaction_weights(), [l0.weight, l0.bias, l1.weight, l1.bias], rep.n_filters, kind, p0, p1,
        rep.cutoff_fn.cutoff_value(), head._head_act)
    if head.aggregation_mode == "avg":
        E = E / inputs[properties.n_atoms]
    inputs["scalar_representation"] = x
    inputs[head.output_key] = E
    return inputs


def _zbl_add(zbl, inputs: Dict[str, torch.Tensor], n_mol: int, F: torch.Tensor, W: Optional[torch.Tensor]) -> torch.Tensor:
    """One operator (four short launches: row pass, chunk and molecule reductions, row pointers of ``idx_m``): the repulsion's forces (and
    virial) added into ``F`` (``W``) in place; returns its energies."""
    R = inputs[properties.R]
    return torch.ops.spk_hip.zbl_forces(R, inputs.get(properties.offsets), inputs[properties.Z], inputs[properties.idx_i], inputs[properties.idx_j],
                                        inputs[properties.idx_m], n_mol, zbl.op_params(R), F, W)


def embedding_table(rep) -> Optional[torch.Tensor]:
    """The table that the force call looks the nuclear embedding rows up in, inside its first launch: the weight of a plain ``nn.Embedding`` or
    the eval table of a ``NuclearEmbedding`` mirror in eval mode -- when there are no electronic embeddings.  None: the caller computes x0."""
    if len(rep.electronic_embeddings) > 0:
        return None
    if type(rep.embedding) is nn.Embedding:
        return rep.embedding.weight
    if type(rep.embedding) is NuclearEmbedding and not rep.embedding.training:
        return rep.embedding.embedding
    return None


def _potential_eval(model, inputs: Dict[str, torch.Tensor], layout: Optional[Tuple[int, int, int, int]], stress: bool) -> Dict[str, torch.Tensor]:
    """The eval body of modes 2 - 5: the one operator that the representation and ``stress`` select, the ZBL repulsion when a ``layout`` is given,
    stress = W / V under ``stress``, then the dict."""
    outs = model.output_modules
    rep, head, frc = model.representation, outs[0], outs[1]
    zbl, agg = None, None
    if layout is not None:
        head, zbl, agg, frc = outs[layout[0]], outs[layout[1]], outs[layout[2]], outs[layout[3]]
    idx_m = inputs[properties.idx_m]
    n_mol = head._n_molecules(inputs, idx_m)
    kind, p0, p1 = rep.radial_basis.kernel_params()
    l0, l1 = head.outnet[0], head.outnet[1]
    table = embedding_table(rep)
    plain = table is not None
    painn = isinstance(rep, PaiNN)
    op = getattr(torch.ops.spk_hip, ("painn" if painn else "schnet") + ("_potential_stress" if stress else "_potential_forces"))
    with torch.no_grad():
        res = list(op(None if plain else rep.embed(inputs), table, inputs[properties.Z], inputs[properties.R],
                      inputs.get(properties.offsets), inputs[properties.idx_i], inputs[properties.idx_j], idx_m, n_mol, rep.interaction_weights(),
                      [l0.weight, l0.bias, l1.weight, l1.bias], *((rep.share_filters, rep.epsilon) if painn else (rep.n_filters,)), kind, p0, p1,
                      rep.cutoff_fn.cutoff_value(), head._head_act))
        E, F, W = res[0], res[1], res[2] if stress else None
        named = {head.output_key: E, frc.force_key: F}
        if zbl is not None:
            named[zbl.output_key] = _zbl_add(zbl, inputs, n_mol, F, W)
            named[agg.output_key] = E + named[zbl.output_key]
        if stress:
            cell = inputs[properties.cell]
            volume = torch.sum(cell[:, 0, :] * torch.cross(cell[:, 1, :], cell[:, 2, :], dim=1), dim=1, keepdim=True)[:, :, None]
            named[frc.stress_key] = W / volume
    if torch.is_grad_enabled():      # a backward pass into this eval-mode model gets the eval-only message, not silence
        named = {k: torch.ops.spk_hip.eval_guard(v, [l0.weight]) for k, v in named.items()}
    inputs["scalar_representation"] = res[-2] if painn else res[-1]
    if painn:
        inputs["vector_representation"] = res[-1]
    inputs.update(named)
    return inputs


def potential_forces_forward(model, inputs: Dict[str, torch.Tensor], layout: Optional[Tuple[int, int, int, int]] = None) -> Dict[str, torch.Tensor]:
    """Energies and forces straight from the two launches (no autograd node: eval only; the embedding rows are looked up
    inside the forward launch when the nuclear embedding is a plain table).  With a ``layout`` (:func:`zbl_layout`, mode 4) the ZBL
    repulsion is added by one more operator and the learned, the repulsion and the aggregated energies are all set."""
    return _potential_eval(model, inputs, layout, False)


def potential_stress_forward(model, inputs: Dict[str, torch.Tensor], layout: Optional[Tuple[int, int, int, int]] = None) -> Dict[str, torch.Tensor]:
    """Energies, forces and stress straight from the operators (eval only, like :func:`potential_forces_forward`): the operator returns the
    virial W = dE/dstrain [n_mol, 3, 3]; stress = W / V with the signed cell volume, as ``Forces`` computes it (atomistic/response.py:81-90).
    ``Strain`` itself does not run: at zero strain it leaves positions, offsets and cell as they are.  With a ``layout`` (mode 5) the ZBL
    repulsion is added into forces and virial by one more operator, as in :func:`potential_forces_forward`."""
    return _potential_eval(model, inputs, layout, True)


def fused_eval_forward(model, inputs: Dict[str, torch.Tensor], mode: int, layout: Optional[Tuple[int, int, int, int]], n_tail: int) -> Dict[str, torch.Tensor]:
    """The route of a :func:`classify_potential` mode 1 - 5 (``layout``: :func:`zbl_layout` for modes 4 / 5, else None), for
    ``NeuralNetworkPotential.forward`` and for the hook that ``install`` puts on the reference's class."""
    if mode == 1:
        inputs = potential_forward(model, inputs)
        for i, m in enumerate(model.output_modules):      # (a tensorial tail is among them)
            if i > 0:
                inputs = m(inputs)
        return inputs
    return run_tail(model, _potential_eval(model, inputs, layout, mode in (3, 5)), n_tail)


def potential_fm_forward(model, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """TRAINING mode of the standard potential: ``torch.ops.spk_hip.schnet_fm`` / ``painn_fm`` -- energies and forces from one
    operator whose backward is the forward-over-reverse engine (csrc/spk_fm.hip): the gradient of any loss(E, F) w.r.t. every
    weight in ~100 launches, where ``Forces(create_graph=True)`` (atomistic/response.py:59-68) records a second-order graph of
    several hundred nodes.  The positions enter detached: the operator differentiates w.r.t. the weights only, the forces it
    returns ARE -dE/dR.  Consequence (documented, not detected: ``forward`` itself marks the positions as requiring grad, like the
    reference's, so a request cannot be told from the default): in train mode the outputs carry no graph to the positions --
    ``autograd.grad(E, R)`` reports an unused input; use ``model.fm_engine = False`` for position derivatives of any order."""
    rep, head, frc = model.representation, model.output_modules[0], model.output_modules[1]
    idx_m = inputs[properties.idx_m]
    kind, p0, p1 = rep.radial_basis.kernel_params()
    l0, l1 = head.outnet[0], head.outnet[1]
    common = (rep.embedding.weight, inputs[properties.Z], inputs[properties.R].detach(), inputs.get(properties.offsets), inputs[properties.idx_i],
              inputs[properties.idx_j], idx_m, head._n_molecules(inputs, idx_m), rep.interaction_weights(), [l0.weight, l0.bias, l1.weight, l1.bias])
    if isinstance(rep, PaiNN):
        E, F = torch.ops.spk_hip.painn_fm(*common, rep.share_filters, rep._eps(), kind, p0, p1, rep.cutoff_fn.cutoff_value(), model._fm_head_act)
    else:
        E, F = torch.ops.spk_hip.schnet_fm(*common, rep.n_filters, kind, p0, p1, rep.cutoff_fn.cutoff_value(), model._fm_head_act)
    inputs[head.output_key] = E
    inputs[frc.force_key] = F
    return inputs


def classify_fm(model) -> int:
    """Activation id of the energy head (> 0) when the force-matching engine covers the model, else 0: ``PairwiseDistances`` -> fused-able
    ``SchNet`` / ``PaiNN`` with a plain nuclear embedding table -> ``Atomwise`` (two Dense layers, width-1 output, summed per molecule; ANY
    hidden width) -> ``Forces`` of that energy without stress.  Looser than :func:`classify_potential`: the engine's Dense layers take any
    width, so e.g. n_atom_basis = 32 (head width 16) trains through it although the fused eval head does not cover it."""
    from . import _lib
    from .nn import Dense
    from .nn.base import activation_id
    rep, ins, outs = model.representation, list(model.input_modules), list(model.output_modules)
    if not (isinstance(rep, (SchNet, PaiNN)) and rep._fused and len(rep.interactions) > 0):
        return 0
    if not (type(rep.embedding) is nn.Embedding and len(rep.electronic_embeddings) == 0):
        return 0
    if getattr(rep.radial_basis, "trainable", False):      # the engine has no gradient w.r.t. offsets / widths: the closed operators do
        return 0
    if not (len(ins) == 1 and type(ins[0]) is PairwiseDistances and len(outs) == 2):
        return 0
    head, frc = outs
    if not (isinstance(head, Atomwise) and head.per_atom_output_key is None and head.aggregation_mode == "sum" and head.n_out == 1):
        return 0
    net = head.outnet
    if not (isinstance(net, nn.Sequential) and len(net) == 2 and all(isinstance(l, Dense) for l in net)):
        return 0
    act = activation_id(net[0].activation)
    if act not in (_lib.SPK_ACT_SSP, _lib.SPK_ACT_SILU) or activation_id(net[1].activation) != _lib.SPK_ACT_NONE:
        return 0
    if net[1].out_features != 1 or net[0].bias is None or net[1].bias is None:
        return 0
    if not (_is_forces(frc) and frc.calc_forces and not frc.calc_stress and frc.energy_key == head.output_key):
        return 0
    return int(act)


class NeuralNetworkPotential(nn.Module):
    """input_modules -> representation -> output_modules (dict in, dict out); TorchScript-able like the reference's
    (src/scripts/spkdeploy:16-40 scripts the whole model).

    The standard potential -- ``PairwiseDistances`` -> fused ``SchNet`` -> ``Atomwise`` (default head, summed or averaged over
    the molecule) -> ``Forces`` without stress -- runs in eval mode as ONE operator, ``torch.ops.spk_hip.schnet_potential``:
    on batches of small molecules the pair vectors, the representation and the energy head are one launch and the backward
    that ``Forces`` triggers (dE/dE -> head -> representation -> dE/dR) is one launch; on every other list the operator runs
    the same three stages through their own kernels.  Any other composition takes the module-by-module path below.
    (``install(fused_potential=True)`` gives the reference's own ``NeuralNetworkPotential`` the same routing.)"""

    required_derivatives: List[str]
    model_outputs: List[str]
    _potential: Final[bool]
    _potential_forces: Final[bool]
    #: eval mode of ``Strain`` -> standard potential -> ``Forces(calc_stress=True)``: energies, forces and stress from one operator
    _potential_stress: bool
    #: training mode of the standard potential through the force-matching engine (``spk_hip::schnet_fm`` / ``painn_fm``: weight
    #: gradients of a loss(E, F) by forward-over-reverse).  Set to False for the operator-by-operator path (any-order autograd).
    fm_engine: bool
    _fm_head_act: int
    #: eval mode of the standard potential with a ZBL repulsion aggregated into the energy (classify_potential 4 / 5): the fused operators
    #: plus one ``zbl_forces`` operator; ``_zbl_layout`` = positions of (head, zbl, aggregation, forces) in ``output_modules``
    _potential_zbl: bool
    _zbl_stress: bool
    _zbl_layout: List[int]

    def __init__(self, representation: nn.Module, input_modules: List[nn.Module] = None,
                 output_modules: List[nn.Module] = None):
        super().__init__()
        self.representation = representation
        self.input_modules = nn.ModuleList(input_modules)
        self.output_modules = nn.ModuleList(output_modules)
        self.required_derivatives = []
        for m in self.modules():
            for p in getattr(m, "required_derivatives", None) or []:
                if p not in self.required_derivatives:
                    self.required_derivatives.append(p)
        outs = []
        for m in self.modules():
            for k in getattr(m, "model_outputs", None) or []:
                if k not in outs:
                    outs.append(k)
        self.model_outputs = outs
        link_charge_consumers(self)
        mode = classify_potential(self)
        self._potential = mode in (1, 2)
        # ... and when the only other output is Forces' -dE/dR, energies AND forces come from the two launches directly
        self._potential_forces = mode == 2
        self._potential_stress = mode == 3
        self._potential_zbl = mode in (4, 5)
        self._zbl_stress = mode == 5
        #: ``DipoleMoment`` / ``Polarizability`` modules at the end of ``output_modules``: they run behind the fused force call
        self._n_tail = tensorial_tail(list(self.output_modules))
        self._zbl_layout = list(zbl_layout(list(self.output_modules)[:len(self.output_modules) - self._n_tail]) or []) if mode in (4, 5) else []
        self._fm_head_act = classify_fm(self)
        self.fm_engine = self._fm_head_act > 0

    def __setstate__(self, state):
        # a model pickled before the ZBL routes existed: it has no such composition
        super().__setstate__(state)
        if "_potential_zbl" not in self.__dict__:
            self._potential_zbl, self._zbl_stress, self._zbl_layout = False, False, []
        if "_n_tail" not in self.__dict__:        # ... or before the tensorial heads
            self._n_tail = 0

    @torch.jit.unused
    def _potential_fm_forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        return potential_fm_forward(self, inputs)

    @torch.jit.unused
    def _fused_forward(self, inputs: Dict[str, torch.Tensor], mode: int) -> Dict[str, torch.Tensor]:
        lay = (self._zbl_layout[0], self._zbl_layout[1], self._zbl_layout[2], self._zbl_layout[3]) if mode in (4, 5) else None
        return fused_eval_forward(self, inputs, mode, lay, self._n_tail)

    @torch.jit.unused
    def _potential_forces_forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        return self._fused_forward(inputs, 2)

    @torch.jit.unused
    def _potential_stress_forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        return self._fused_forward(inputs, 3)

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        for p in self.required_derivatives:
            if p in inputs:
                inputs[p].requires_grad_()
        dev_ok = properties.R in inputs and (inputs[properties.R].is_cuda or inputs[properties.R].is_meta) and inputs[properties.R].dtype == torch.float32
        if not dev_ok:           # host / non-float32 tensors: module by module, every mirror on its ATen route (nn/fallback.py)
            for m in self.input_modules:
                inputs = m(inputs)
            inputs = self.representation(inputs)
            for m in self.output_modules:
                inputs = m(inputs)
            return {k: inputs[k] for k in self.model_outputs}
        # the route, from the flags as they are at this call (callers toggle them): forces, stress, zbl, then mode 1; training has the engine below
        mode = 0
        if not self.training and not torch.jit.is_scripting():
            if self._potential_forces:
                mode = 2
            elif self._potential_stress:
                mode = 3
            elif self._potential_zbl:
                mode = 5 if self._zbl_stress else 4
            elif self._potential:
                mode = 1
        if mode > 0:
            inputs = self._fused_forward(inputs, mode)
            return {k: inputs[k] for k in self.model_outputs}
        if self.training and self.fm_engine and not torch.jit.is_scripting():
            pos = inputs[properties.R]
            w0 = self.representation.embedding.weight
            # the engine is fp32 on the device, for positions AND parameters; anything else (float64 checks of the operator-by-operator path on
            # the host, float64 weights) takes the primitives below
            if pos.is_cuda and pos.dtype == torch.float32 and w0.is_cuda and w0.dtype == torch.float32:
                inputs = self._potential_fm_forward(inputs)
                return {k: inputs[k] for k in self.model_outputs}
        for m in self.input_modules:
            inputs = m(inputs)
        inputs = self.representation(inputs)
        for m in self.output_modules:
            inputs = m(inputs)
        return {k: inputs[k] for k in self.model_outputs}


def build_model(kind: str = "schnet", n_atom_basis: int = 128, n_interactions: int = 3,
                n_rbf: int = 20, cutoff: float = 5.0, radial: str = "gaussian", trainable_rbf: bool = False, **rep_kw):
    """SchNet / PaiNN + Atomwise energy head + Forces, assembled like
    configs/model/nnp.yaml:4-8 + experiment/md17.yaml:30-38."""
    rb = GaussianRBF(n_rbf, cutoff, trainable=trainable_rbf) if radial == "gaussian" else BesselRBF(n_rbf, cutoff)
    cf = CosineCutoff(cutoff)
    if kind == "schnet":
        rep = SchNet(n_atom_basis, n_interactions, rb, cf, **rep_kw)
    elif kind == "painn":
        rep = PaiNN(n_atom_basis, n_interactions, rb, cf, **rep_kw)
    else:
        raise ValueError(kind)
    return NeuralNetworkPotential(rep, input_modules=[PairwiseDistances()],
                                  output_modules=[Atomwise(n_in=n_atom_basis, output_key=properties.energy),
                                                  Forces()])


def load_reference_params(model: NeuralNetworkPotential, rep_params, head_params):
    """Load parameters given with the reference's state_dict key names (representation keys and
    ``outnet.*`` head keys)."""
    sd = model.representation.state_dict()
    missing = [k for k in sd if k not in rep_params]
    if missing:
        raise KeyError("missing representation parameters: %s" % missing)
    model.representation.load_state_dict({k: rep_params[k].to(sd[k].dtype) for k in sd})
    model.output_modules[0].load_state_dict({k: v for k, v in head_params.items()})
    return model


def batch_to_inputs(batch, device) -> Dict[str, torch.Tensor]:
    """Synthetic batch (schnetpack_amd.synthetic) -> the reference's input dict on ``device``."""
    inp = {
        properties.Z: batch["Z"].to(device),
        properties.R: batch["R"].to(device).float().clone(),
        properties.idx_i: batch["idx_i"].to(device),
        properties.idx_j: batch["idx_j"].to(device),
        properties.offsets: batch["offsets"].to(device).float(),
        properties.idx_m: batch["idx_m"].to(device),
        "_n_molecules": int(batch["n_mol"]),
    }
    return inp
