"""Drop-in hook: route the reference package's hot-path names to the HIP-backed mirrors.

    import schnetpack, schnetpack_amd.install
    schnetpack_amd.install.install()          # before building / unpickling a model

Patches, inside the already imported ``schnetpack`` package, exactly the names of SURVEY.md
section 8(b): ``nn.scatter_add`` (+ ``nn.scatter.scatter_add``), ``nn.Dense``, ``nn.GaussianRBF``,
``nn.BesselRBF``, ``nn.CosineCutoff``, ``representation.{SchNet, SchNetInteraction, PaiNN,
PaiNNInteraction, PaiNNMixing}``, ``atomistic.PairwiseDistances``, ``atomistic.ZBLRepulsionEnergy``,
``atomistic.Aggregation``, ``nn.GatedEquivariantBlock``, ``nn.build_gated_equivariant_mlp``,
``atomistic.{DipoleMoment, Polarizability}``, ``nn.SwitchFunction``, ``atomistic.FilterShortRange`` and
``atomistic.{CoulombPotential, DampedCoulombPotential, EnergyCoulomb, EnergyEwald}``, ``nn.so3.{RealSphericalHarmonics, scalar2rsh,
SO3TensorProduct, SO3Convolution, SO3ParametricGatedNonlinearity, SO3GatedNonlinearity}`` (+ the names ``nn`` re-exports) and
``representation.SO3net``.  Classes are replaced both on
the package and on the defining sub-module, so Hydra ``_target_`` paths and pickled models
(``torch.load`` resolves ``schnetpack.representation.painn.PaiNN`` by attribute) pick up the
mirrors; parameter names and shapes are identical, so existing ``state_dict``s and whole-model
pickles load unchanged.  Everything else of the reference (Atomwise, Forces, AtomisticModel,
spktrain, md.Simulator, ...) keeps running its own code on top.
"""
import importlib
import sys

import torch


_ORIGINALS = []      # (module, name, original object) in patch order, for uninstall()


def _set(mod, name, obj, log):
    if mod is not None and hasattr(mod, name):
        if getattr(mod, name) is not obj:
            _ORIGINALS.append((mod, name, getattr(mod, name)))
        setattr(mod, name, obj)
        log.append("%s.%s" % (mod.__name__, name))


def uninstall():
    """Undo every ``install()`` of this process: the reference's own classes / functions are put back
    (models built or unpickled in between keep the classes they were made from)."""
    n = len(_ORIGINALS)
    while _ORIGINALS:
        mod, name, orig = _ORIGINALS.pop()
        if orig is _ABSENT:
            if hasattr(mod, name):
                delattr(mod, name)
        else:
            setattr(mod, name, orig)
    return n


_ABSENT = object()


def _fused_potential_call(orig_call):
    """``NeuralNetworkPotential.__call__`` with the standard potential handed to the fused operators (model.classify_potential):
    an eval-mode call of a model that is PairwiseDistances -> SchNet / PaiNN -> default Atomwise -> Forces runs as the two-launch
    operator; everything else -- training mode, any other composition, a model with forward hooks, keyword / extra arguments --
    goes through ``nn.Module.__call__`` to the reference's own ``forward`` (model/base.py:174-190), which is NOT touched: the class
    stays scriptable (``torch.jit.script`` compiles ``forward``; ``spkdeploy`` and the LAMMPS route depend on it), and a scripted
    module has its own ``__call__``.  The classification of an instance is made once."""
    from . import model as M

    def __call__(self, *args, **kwargs):
        if "_spk_hip_linked" not in self.__dict__:      # predicted charges that a later electrostatic term reads: differentiable in eval mode too
            self.__dict__["_spk_hip_linked"] = M.link_charge_consumers(self)
        if (self.training or len(args) != 1 or kwargs or not isinstance(args[0], dict)
                or self._forward_hooks or self._forward_pre_hooks):
            return orig_call(self, *args, **kwargs)
        pos = args[0].get("_positions")
        if not (torch.is_tensor(pos) and (pos.is_cuda or pos.is_meta) and pos.dtype == torch.float32):
            # host / non-float32 tensors (e.g. BASELINE configs[0]: a CPU force evaluation): the reference's own forward, every mirror
            # module on its ATen route (nn/fallback.py)
            return orig_call(self, *args, **kwargs)
        mode = self.__dict__.get("_spk_hip_mode")
        if mode is None:
            mode = M.classify_potential(self)
            self.__dict__["_spk_hip_mode"] = mode
        if mode == 0:
            return orig_call(self, *args, **kwargs)
        inputs = self.initialize_derivatives(args[0])
        n_tail = self.__dict__.get("_spk_hip_tail")
        if n_tail is None:      # DipoleMoment / Polarizability mirrors at the end of output_modules: they run behind the fused call
            n_tail = M.tensorial_tail(list(self.output_modules))
            self.__dict__["_spk_hip_tail"] = n_tail
        lay = None
        if mode in (4, 5):      # ... with a ZBL repulsion aggregated into the energy: one more launch
            lay = self.__dict__.get("_spk_hip_zbl")
            if lay is None:
                lay = M.zbl_layout(list(self.output_modules)[:len(self.output_modules) - n_tail])
                self.__dict__["_spk_hip_zbl"] = lay
        inputs = M.fused_eval_forward(self, inputs, mode, lay, n_tail)
        inputs = self.postprocess(inputs)
        return self.extract_outputs(inputs)

    __call__._spk_hip_patched = True
    return __call__


def install(spk=None, verbose=False, fused_head=True, neighbor_lists=False, fused_potential=True):
    """Patch ``spk`` (default: the imported ``schnetpack``).  Returns the list of patched names.

    ``fused_head`` (default on) also routes ``atomistic.Atomwise`` to the mirror whose default 2-layer energy head
    runs as one fused kernel pair in eval mode (same constructor, ``state_dict`` keys and outputs).
    ``fused_potential`` (default on since round 4; needs ``fused_head``) wraps ``model.base.NeuralNetworkPotential.__call__``:
    an eval-mode call of a model that is the standard potential (PairwiseDistances -> SchNet / PaiNN -> default Atomwise ->
    Forces) runs as the two-launch operator exactly like the mirror model -- 1.3-2 x the module-by-module route; any other
    model, training, and ``torch.jit.script`` (the class ``forward`` is untouched) keep the reference's code.
    ``install(fused_head=False, fused_potential=False)`` is the minimal patch of rounds 1-3 -- plus, since the ZBL kernels exist,
    ``atomistic.ZBLRepulsionEnergy`` and ``atomistic.Aggregation`` (same constructors, ``state_dict`` keys and ATen formulas; patched in every
    configuration, when the reference has loaded those modules).
    ``neighbor_lists=True`` adds ``transform.HipNeighborList`` and replaces ``md.neighborlist_md.NeighborListMD``
    by the device-side batched version (same constructor and ``get_neighbors``)."""
    from . import atomistic as A
    from . import nn as N
    from . import representation as R
    if spk is None:
        spk = sys.modules.get("schnetpack") or importlib.import_module("schnetpack")

    def sub(path):
        return sys.modules.get(spk.__name__ + "." + path)

    log = []
    for mod in (getattr(spk, "nn", None), sub("nn.scatter")):
        _set(mod, "scatter_add", N.scatter_add, log)
    for mod in (getattr(spk, "nn", None), sub("nn.base")):
        _set(mod, "Dense", N.Dense, log)
    for mod in (getattr(spk, "nn", None), sub("nn.radial")):
        _set(mod, "GaussianRBF", N.GaussianRBF, log)
        _set(mod, "BesselRBF", N.BesselRBF, log)
    for mod in (getattr(spk, "nn", None), sub("nn.cutoff")):
        _set(mod, "CosineCutoff", N.CosineCutoff, log)
    for mod in (getattr(spk, "representation", None), sub("representation.schnet")):
        _set(mod, "SchNet", R.SchNet, log)
        _set(mod, "SchNetInteraction", R.SchNetInteraction, log)
    for mod in (getattr(spk, "representation", None), sub("representation.painn")):
        _set(mod, "PaiNN", R.PaiNN, log)
        _set(mod, "PaiNNInteraction", R.PaiNNInteraction, log)
        _set(mod, "PaiNNMixing", R.PaiNNMixing, log)
    for mod in (getattr(spk, "atomistic", None), sub("atomistic.distances")):
        _set(mod, "PairwiseDistances", A.PairwiseDistances, log)
    # modules that did `from schnetpack.nn import scatter_add` / `import schnetpack.nn as snn` keep
    # working: the first form is re-bound here, the second resolves the attribute at call time
    for name in ("atomistic.atomwise", "nn.so3", "atomistic.electrostatic", "atomistic.nuclear_repulsion"):
        m = sub(name)
        if m is not None and getattr(m, "scatter_add", None) is not None:
            _set(m, "scatter_add", N.scatter_add, log)
    if fused_head:
        for mod in (getattr(spk, "atomistic", None), sub("atomistic.atomwise")):
            _set(mod, "Atomwise", A.Atomwise, log)
    # the ZBL repulsion and the sum of energies (when the reference has loaded them): same constructors and state_dict keys
    for mod in (getattr(spk, "atomistic", None), sub("atomistic.nuclear_repulsion")):
        _set(mod, "ZBLRepulsionEnergy", A.ZBLRepulsionEnergy, log)
    for mod in (getattr(spk, "atomistic", None), sub("atomistic.aggregation")):
        _set(mod, "Aggregation", A.Aggregation, log)
    # the tensorial heads and the gated equivariant blocks they are made of (when the reference has loaded them)
    for mod in (getattr(spk, "nn", None), sub("nn.equivariant")):
        _set(mod, "GatedEquivariantBlock", N.GatedEquivariantBlock, log)
    for mod in (getattr(spk, "nn", None), sub("nn.blocks")):
        _set(mod, "build_gated_equivariant_mlp", N.build_gated_equivariant_mlp, log)
    for mod in (getattr(spk, "atomistic", None), sub("atomistic.atomwise")):
        _set(mod, "DipoleMoment", A.DipoleMoment, log)
        _set(mod, "Polarizability", A.Polarizability, log)
    # point-charge electrostatics (when the reference has loaded them): same constructors, buffers and state_dict keys
    for mod in (getattr(spk, "nn", None), sub("nn.cutoff")):
        _set(mod, "SwitchFunction", N.SwitchFunction, log)
    for mod in (getattr(spk, "atomistic", None), sub("atomistic.distances")):
        _set(mod, "FilterShortRange", A.FilterShortRange, log)
    for mod in (getattr(spk, "atomistic", None), sub("atomistic.electrostatic")):
        for name in ("CoulombPotential", "DampedCoulombPotential", "EnergyCoulomb", "EnergyEwald"):
            _set(mod, name, getattr(A, name), log)
    # the SO(3) layers and SO3net (when the reference has loaded them): same constructors, buffers and state_dict keys
    from .nn import so3 as S3
    for mod in (getattr(spk, "nn", None), sub("nn.so3")):
        for name in ("RealSphericalHarmonics", "scalar2rsh", "SO3TensorProduct", "SO3Convolution", "SO3ParametricGatedNonlinearity",
                     "SO3GatedNonlinearity"):
            _set(mod, name, getattr(S3, name), log)
    for mod in (getattr(spk, "representation", None), sub("representation.so3net")):
        _set(mod, "SO3net", R.SO3net, log)
    # the nuclear / electronic embeddings and their residual blocks (when the reference has loaded them): same constructors, buffers and state_dict keys
    for mod in (getattr(spk, "nn", None), sub("nn.embedding")):
        _set(mod, "NuclearEmbedding", N.NuclearEmbedding, log)
        _set(mod, "ElectronicEmbedding", N.ElectronicEmbedding, log)
    for mod in (getattr(spk, "nn", None), sub("nn.blocks")):
        for name in ("Residual", "ResidualStack", "ResidualMLP"):
            _set(mod, name, getattr(N, name), log)
    for mod in (sub("nn.embedding"),):      # (it did `from schnetpack.nn.blocks import ResidualMLP`)
        _set(mod, "ResidualMLP", N.ResidualMLP, log)
    if fused_potential and fused_head:
        mb = sub("model.base")
        cls = getattr(mb, "NeuralNetworkPotential", None) if mb is not None else None
        if cls is not None and not getattr(cls.__call__, "_spk_hip_patched", False):
            # (the patched name is the class's own __call__ attribute: absent before, nn.Module's is inherited)
            _ORIGINALS.append((cls, "__call__", cls.__dict__.get("__call__", _ABSENT)))
            cls.__call__ = _fused_potential_call(cls.__call__)
            log.append(mb.__name__ + ".NeuralNetworkPotential.__call__")
    if neighbor_lists:
        from . import neighborlist as NL
        for mod in (getattr(spk, "transform", None), sub("transform.neighborlist")):
            if mod is not None:
                if not hasattr(mod, "HipNeighborList"):
                    _ORIGINALS.append((mod, "HipNeighborList", _ABSENT))
                setattr(mod, "HipNeighborList", NL.HipNeighborList)
                log.append(mod.__name__ + ".HipNeighborList")
        for mod in (sub("md"), sub("md.neighborlist_md")):
            _set(mod, "NeighborListMD", NL.NeighborListMD, log)
    if verbose:
        print("schnetpack_amd.install: patched", ", ".join(log))
    return log
