"""Stress from the standard potential, host side: classification of the Strain composition, the mirror ``Strain`` against the
reference's on the ATen route (fp64, triclinic cells), the deployed file of a stress model, the C ABI of the virial and the register
budget of its kernels."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import refshim
from schnetpack_amd import model as M, synthetic as S
from schnetpack_amd.atomistic import Atomwise, Forces, PairwiseDistances, Strain
from schnetpack_amd.csrc import build as B


def _stress_model(kind, strain=None, radial="gaussian"):
    base = M.build_model(kind, radial=radial)
    ins = [strain if strain is not None else Strain(), PairwiseDistances()]
    return M.NeuralNetworkPotential(base.representation, input_modules=ins,
                                    output_modules=[base.output_modules[0], Forces(calc_forces=True, calc_stress=True)])


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_classify_strain_composition(kind):
    m = _stress_model(kind)
    assert M.classify_potential(m) == 3 and m._potential_stress and not m._potential and not m._potential_forces
    # without Strain, stress keeps the module-by-module route
    plain = M.build_model(kind)
    plain.output_modules[1].calc_stress = True
    assert M.classify_potential(plain) == 0
    # Strain without stress, stress without forces, an averaged head, an extra output: not the standard potential
    m.output_modules[1].calc_stress = False
    assert M.classify_potential(m) == 0
    m = _stress_model(kind)
    m.output_modules[1].calc_forces = False
    assert M.classify_potential(m) == 0
    m = _stress_model(kind)
    m.output_modules[0].aggregation_mode = "avg"
    assert M.classify_potential(m) == 0
    m = _stress_model(kind)
    m.input_modules = torch.nn.ModuleList([PairwiseDistances(), Strain()])
    assert M.classify_potential(m) == 0


def test_periodic_molecule_batch_layout():
    b = S.periodic_molecule_batch("aspirin", 4, edge=11.0, tilt=0.2, seed=3)
    assert b["cell"].shape == (4, 3, 3) and b["n_mol"] == 4
    assert float(b["cell"][1, 1, 0]) != 0.0 and float(b["cell"][0, 1, 0]) == 0.0       # mixed cubic / triclinic
    ii, jj = b["idx_i"].numpy(), b["idx_j"].numpy()
    key = ii * len(b["Z"]) + jj
    assert (np.diff(key) > 0).all()                                                     # sorted, one image per pair
    assert (b["idx_m"][ii] == b["idx_m"][jj]).all()                                     # block-diagonal by frame
    assert (b["offsets"].abs().sum(1) > 0).any()                                        # images do occur
    pos = {(a, c): o for a, c, o in zip(ii, jj, b["offsets"].numpy())}
    assert all(np.array_equal(pos[(c, a)], -o) for (a, c), o in pos.items())           # symmetric
    with pytest.raises(ValueError):
        S.periodic_molecule_batch("aspirin", 2, edge=10.5)


def _inputs(b, dtype=torch.float64):
    return {"_atomic_numbers": b["Z"], "_positions": b["R"].to(dtype).clone(), "_idx_i": b["idx_i"], "_idx_j": b["idx_j"],
            "_offsets": b["offsets"].to(dtype).clone(), "_idx_m": b["idx_m"], "_cell": b["cell"].reshape(-1, 3, 3).to(dtype).clone(),
            "_n_molecules": int(b["n_mol"])}


@pytest.mark.skipif(not refshim.available(), reason="neither the reference package nor oracle/_ref present")
@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_mirror_strain_equals_reference_on_host(kind):
    ns = refshim.load()
    b = S.periodic_molecule_batch("aspirin", 4, edge=11.0, tilt=0.25, seed=5)
    torch.manual_seed(0)
    mine = _stress_model(kind).double().eval()
    ref = _stress_model(kind, strain=ns.response.Strain()).double().eval()
    ref.load_state_dict(mine.state_dict())
    out_m, out_r = mine(_inputs(b)), ref(_inputs(b))
    assert out_m["stress"].shape == (4, 3, 3)
    for k in ("energy", "forces", "stress"):
        err = float((out_m[k] - out_r[k]).abs().max() / out_r[k].abs().max())
        assert err < 1e-10, (k, err)
    # the stress is not trivially zero, and the triclinic frames carry it too
    assert float(out_m["stress"][1].abs().max()) > 1e-6


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_export_of_stress_model_equals_stress_free_export(kind):
    from schnetpack_amd import deploy
    torch.manual_seed(1)
    m = _stress_model(kind).eval()
    plain = M.NeuralNetworkPotential(m.representation, input_modules=[PairwiseDistances()],
                                     output_modules=[m.output_modules[0], Forces()]).eval()
    assert deploy.export_potential(m) == deploy.export_potential(plain)
    # stress without a Strain module has nothing to differentiate against
    plain.output_modules[1].calc_stress = True
    with pytest.raises(ValueError, match="Strain"):
        deploy.export_potential(plain)


def test_lib_binds_virial_symbols():
    from schnetpack_amd import _lib
    L = _lib.lib()
    for name in ("spk_edge_virial_f32", "spk_edge_virial_workspace_bytes", "spk_schnet_potential_forces_gr_f32", "spk_painn_potential_gr_f32",
                 "spk_potential_compute_virial", "spk_potential_compute_cell_virial"):
        fn = getattr(L, name)
        assert fn.argtypes is not None, name
    from schnetpack_amd import torchops
    assert "schnet_potential_stress" in torchops.OPERATORS and "painn_potential_stress" in torchops.OPERATORS


def test_virial_workspace_size_host_query():
    from schnetpack_amd import _lib
    g = _lib.GraphT()
    g.n_atoms, g.n_edges, g.sorted = 100, 1000, 1
    g.rowptr = 1                                   # (only its presence is read)
    sorted_bytes = _lib.lib().spk_edge_virial_workspace_bytes(g, 4, 0)
    g.sorted, g.rowptr = 0, None
    unsorted_bytes = _lib.lib().spk_edge_virial_workspace_bytes(g, 4, 0)
    assert 0 < sorted_bytes < unsorted_bytes
    assert _lib.lib().spk_edge_virial_workspace_bytes(g, 4, 1) < unsorted_bytes    # W_atom given by the caller: no own copy


def test_virial_kernels_have_no_scratch():
    path = os.path.join(B.HERE, "spk_virial.hip")
    cmd = [B._hipcc()] + B.flags_for(path) + ["-c", path, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900).stderr
    rows, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark: [^ ]+ +(?:Function Name|Name): (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    for frag in ("k_edge_virial_row", "k_virial_chunk", "k_virial_mol"):
        hits = [v for k, v in rows.items() if frag in k]
        assert len(hits) == 1, (frag, sorted(rows))
        assert hits[0]["scratch"] == 0 and hits[0]["occ"] >= 4, (frag, hits[0])
