"""Generator of tests/golden/deploy_parent_blobs.npz (a plain script, not collected by pytest):

    python tests/make_deploy_parent_golden.py path/to/deploy.py

``path/to/deploy.py`` is ``schnetpack_amd/deploy.py`` of the commit BEFORE the optional ``zbl`` tensor existed (``git show <commit>:schnetpack_amd/deploy.py``).
Its ``export_potential`` is run on models whose weights do not depend on a random generator: two small ones filled by an integer formula
(:func:`formula_model`; their files are stored whole, as uint8) and the two reference-trained PaiNN models of tests/golden/deploy_painn.npz (files
of 2 MB: stored as SHA-256 and length).  tests/test_zbl_reference.py asserts that today's ``export_potential`` writes the same bytes."""
import hashlib
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.make_golden import save_npz_reproducible  # noqa: E402
from schnetpack_amd import model as M  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "deploy_parent_blobs.npz")


def formula_model(kind):
    """SchNet / PaiNN (64 features, one interaction, 8 radial functions) + head + Forces with every parameter set to
    ((7919 i + 104729 k) mod 1000) / 5000 - 0.1 for element i of the k-th parameter: exact in float32, the same on every machine."""
    m = M.build_model(kind, 64, 1, 8, 4.0)
    with torch.no_grad():
        for k, (_, p) in enumerate(m.named_parameters()):
            i = torch.arange(p.numel(), dtype=torch.int64)
            p.copy_((((7919 * i + 104729 * k) % 1000).double() / 5000.0 - 0.1).float().reshape(p.shape))
    return m.eval()


def golden_models():
    from conftest import load_npz
    from test_deploy import _painn_from_golden
    g, gp = load_npz("deploy_painn.npz"), load_npz("painn_aspirin_pretrained.npz")
    return {"aspirin": _painn_from_golden("w_rep.", "w_head.", gp, int(g["aspirin_n_interactions"]), float(g["aspirin_cutoff"]), float(g["aspirin_mean"])),
            "ethanol": _painn_from_golden("ethanol_w_rep.", "ethanol_w_head.", g, int(g["ethanol_n_interactions"]), float(g["ethanol_cutoff"]),
                                          float(g["ethanol_mean"]))}


def main():
    spec = importlib.util.spec_from_file_location("schnetpack_amd._deploy_before", sys.argv[1])
    before = importlib.util.module_from_spec(spec)
    before.__package__ = "schnetpack_amd"
    spec.loader.exec_module(before)
    arrs = {}
    for kind in ("schnet", "painn"):
        blob = before.export_potential(formula_model(kind))
        arrs["formula_" + kind] = np.frombuffer(blob, dtype=np.uint8)
        print("formula_%s: %d bytes" % (kind, len(blob)))
    for name, m in golden_models().items():
        blob = before.export_potential(m)
        arrs[name + "_sha256"] = np.asarray(hashlib.sha256(blob).hexdigest())
        arrs[name + "_bytes"] = np.asarray(len(blob), dtype=np.int64)
        print("%s: %d bytes %s" % (name, len(blob), hashlib.sha256(blob).hexdigest()))
    save_npz_reproducible(OUT, arrs)
    print("wrote %s, %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
