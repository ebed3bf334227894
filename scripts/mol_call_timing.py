"""Eval force call of SchNet on three batches of small groups: HIP-event time per call (median of 10 replays of a graph of 50 calls) and the
two launches alone (library profile, 20 eager calls).  The control of a change to the molecule-resident kernels: run it once per build.

    python scripts/mol_call_timing.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
import torch
from schnetpack_amd import _lib, data as D, model as M, synthetic as S
dev = torch.device("cuda:0")
torch.manual_seed(0)
m = M.build_model("schnet").to(dev).eval()
CALLS, RUNS = 50, 10

for name, batch in (("ethanol x 256", S.molecule_batch("ethanol", 256, seed=0)), ("aspirin x 256", S.molecule_batch("aspirin", 256, seed=0)),
                    ("blob_molecule_batch(16, 256, seed=16)", S.blob_molecule_batch(16, 256, seed=16))):
    plan = D.host_plan(batch["idx_i"].numpy(), batch["idx_j"].numpy(), batch["offsets"].numpy(), int(batch["Z"].shape[0]))
    tiles = (np.diff(plan["grp_pair0"].astype(np.int64)) + 31) // 32
    inp = M.batch_to_inputs(batch, dev)
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(dict(inp))
    torch.cuda.current_stream().wait_stream(side); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            m(dict(inp))
    g.replay(); torch.cuda.synchronize()
    t = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); g.replay(); b.record(); b.synchronize()
        t.append(1e3 * a.elapsed_time(b) / CALLS)
    _lib.profile_enable(True); _lib.profile_report()
    for _ in range(20):
        m(dict(inp))
    k = {tag: round(1e3 * v[1] / v[0], 2) for tag, v in _lib.profile_report().items()}
    _lib.profile_enable(False)
    v = np.array(t)
    print("%s: %d groups, tiles per group min/median/max %d %d %d: us per call median %.2f  min %.2f  max %.2f   kernels (us) %s" % (
        name, tiles.shape[0], tiles.min(), np.median(tiles), tiles.max(), np.median(v), v.min(), v.max(), k))
