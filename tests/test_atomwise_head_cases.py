"""The layouts of tests/atomwise_head_cases.py have the properties their names claim, its float64 formula agrees with autograd on an
independent formulation, its dispatch predicate has the edges of spk_atomwise_fwd_f32, and the cases are well-conditioned: the same
formula in float32 on the host stays below half the bound tests/test_gpu_atomwise_head.py holds the device to (1e-5 against float64)
on every shape, layout and activation that file runs -- a device failure on them cannot be blamed on the inputs.  No GPU.  The
figures are printed."""
import pytest
import torch

import atomwise_head_cases as A

TOL = 1e-5
N_CU = 256                       # compute units of an MI355X; the GPU file reads the count of the device it runs on
NS = sorted(set(A.TILE_NS + A.BWD_NS + (200, 333) + A.edge_ns(N_CU) + A.edge_ns(8)))


# ---------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.LAYOUTS)
def test_ids_are_in_range_and_seeded(name):
    for N in [0] + NS:
        idx, n_mol = A.layout(name, N)
        assert idx.dtype == torch.int64 and idx.shape == (N,) and n_mol >= 1
        if N:
            assert int(idx.min()) >= 0 and int(idx.max()) < n_mol, (name, N)
        again, n2 = A.layout.__wrapped__(name, N)
        assert n2 == n_mol and torch.equal(idx, again)


def test_one_each_ragged_descending():
    for N in NS:
        one, n1 = A.layout("one", N)
        assert n1 == 1 and (one == 0).all()
        each, ne = A.layout("each", N)
        assert ne == N and torch.equal(each, torch.arange(N))
        for s in range(0, N - A.BLOCK32 + 1, A.BLOCK32):          # 128 distinct ids per 128 atoms: every LDS slot of a block
            blk = each[s:s + A.BLOCK32] - each[s]
            assert torch.equal(blk, torch.arange(A.SLOTS))
        rag, nr = A.layout("ragged", N)
        assert (rag[1:] - rag[:-1] >= 0).all() and (rag[1:] - rag[:-1] <= 1).all() and int(rag[0]) == 0 and int(rag[-1]) == nr - 1
        sizes = torch.bincount(rag, minlength=nr)
        assert int(sizes.min()) >= 1 and int(sizes.max()) <= 39
        des, nd = A.layout("descending", N)
        assert nd == nr and torch.equal(torch.flip(des, [0]), rag)
        if nr > 1:                                                 # rel < 0 for every later molecule of the first workgroup
            assert int((des - des[0]).min()) < 0
    sizes = torch.bincount(A.layout("ragged", 32 * N_CU)[0])
    assert int(sizes.min()) == 1 and int(sizes.max()) == 39 and len(sizes) > A.SLOTS


def test_gaps_leaves_ids_empty_at_the_front_inside_and_at_the_end():
    for N in NS:
        idx, n_mol = A.layout("gaps", N)
        assert (idx[1:] - idx[:-1] >= 0).all()
        used = torch.unique(idx)
        want = [1, 4, 5, 9, 12, 13, 17, 20, 21, 25]
        assert used[:len(want)].tolist() == want[:len(used)], (N, used[:10])
        assert n_mol == int(used[-1]) + 4
        empty = A.empty_ids({"idx_m": idx, "n_mol": n_mol}).tolist()
        assert 0 in empty and empty[-3:] == [n_mol - 3, n_mol - 2, n_mol - 1]
        if len(used) > 1:
            assert any(int(used[0]) < e < int(used[-1]) for e in empty), N
        assert int(torch.bincount(idx)[used].max()) <= 5
    assert len(torch.unique(A.layout("gaps", 15)[0])) >= 3           # the smallest tile-edge count already has all three kinds


def test_interleaved_puts_a_molecule_in_several_segments_of_every_full_tile():
    for N in NS:
        idx, n_mol = A.layout("interleaved", N)
        assert n_mol == 3
        for t in range(N // A.TILE16):
            seg = A.segments(idx[A.TILE16 * t:A.TILE16 * (t + 1)])
            assert len(seg) == A.TILE16                            # every atom ends a segment: 16 "last" lanes on 3 slots
            for m in range(3):
                assert sum(1 for a, _ in seg if a == m) >= 2, (N, t, m)


@pytest.mark.parametrize("n_cu", [8, 104, 256, 304])
def test_far_reaches_past_the_lds_slots_of_every_workgroup(n_cu):
    for N in [n for n in NS if n >= 200] + list(A.edge_ns(n_cu)):
        idx, n_mol = A.layout("far", N)
        rag, nr = A.layout("ragged", N)
        assert n_mol >= 200 and n_mol == nr + 200
        last = torch.arange(A.TILE16 - 1, N, A.TILE16)
        assert (idx[last] == n_mol - 1).all()
        keep = torch.ones(N, dtype=torch.bool)
        keep[last] = False
        assert torch.equal(idx[keep], rag[keep])
        for kernel in ("fwd16", "fwd32"):
            starts = A.block_starts(kernel, N, n_cu)
            assert starts[0] == 0 and all(s % A.TILE16 == 0 for s in starts)
            for s, e in zip(starts, starts[1:] + [N]):
                if e - s >= A.TILE16:
                    assert int((idx[s:e] - idx[s]).max()) >= A.SLOTS, (kernel, N, s)
        empty = A.empty_ids({"idx_m": idx, "n_mol": n_mol})
        assert len(empty) >= 199
    assert A.layout("far", 129)[1] == A.layout("ragged", 129)[1] + 1


def test_block_starts_follow_the_launchers():
    assert A.block_starts("fwd32", 129, 256) == [0, 128]
    assert A.block_starts("fwd16", 129, 256) == list(range(0, 129, 16))
    assert A.block_starts("fwd16", 32 * 8, 8) == list(range(0, 256, 16))          # 16 tiles on 16 workgroup slots
    assert A.block_starts("fwd16", 33 * 16, 8) == list(range(0, 33 * 16, 48))     # 33 tiles: 3 per workgroup


# ---------------------------------------------------------------------------------------------------------
# dispatch predicate
# ---------------------------------------------------------------------------------------------------------
def test_takes_fwd16_at_its_edges():
    for n_cu in (8, 256, 304):
        lo, hi = A.edge_ns(n_cu)
        assert A.takes_fwd16(128, 64, lo, n_cu) and not A.takes_fwd16(128, 64, hi, n_cu)
        assert A.takes_fwd16(128, 64, lo - 15, n_cu) and A.takes_fwd16(128, 64, 1, n_cu)
    assert A.takes_fwd16(128, 32, 17, N_CU) and A.takes_fwd16(128, 64, 17, N_CU)
    assert not A.takes_fwd16(128, 96, 17, N_CU) and not A.takes_fwd16(192, 128, 17, N_CU) and not A.takes_fwd16(128, 160, 17, N_CU)
    assert A.takes_fwd16(512, 64, 17, N_CU) and not A.takes_fwd16(544, 64, 17, N_CU)
    assert not A.takes_fwd16(128, 64, 17, N_CU, b1_aligned=False)
    assert not A.takes_fwd16(128, 64, 17, N_CU, simple=True)
    assert all(A.takes_fwd16(i, h, n, N_CU) for i, h in A.FWD16_SHAPES for n in A.TILE_NS + A.both_kernel_ns(N_CU))
    assert not any(A.takes_fwd16(i, h, n, N_CU) for i, h in A.FWD32_SHAPES for n in A.TILE_NS)


# ---------------------------------------------------------------------------------------------------------
# the formula
# ---------------------------------------------------------------------------------------------------------
def test_inputs_are_float32_values_with_the_stated_scales():
    c = A.make_case(128, 64, 8193, "ragged")
    for k in ("x", "w1", "b1", "w2", "b2", "wE", "wA"):
        assert c[k].dtype == torch.float64 and torch.equal(c[k], c[k].float().double()), k
    assert c["x"].shape == (8193, 128) and c["w1"].shape == (64, 128) and c["b1"].shape == (64,) and c["w2"].shape == (64,)
    assert c["wE"].shape == (c["n_mol"],) and c["wA"].shape == (8193,) and float(c["b2"]) == 0.5
    assert abs(float(c["x"].std()) - 1) < 0.02 and abs(float(c["w1"].std()) * 128 ** 0.5 - 1) < 0.05
    other = A.make_case(128, 64, 8193, "interleaved")
    assert torch.equal(c["x"], other["x"]) and torch.equal(c["w1"], other["w1"])     # a shape's layouts share the head


@pytest.mark.parametrize("act", A.ACTS)
@pytest.mark.parametrize("name", A.LAYOUTS)
def test_oracle_agrees_with_autograd_on_an_independent_formulation(name, act):
    """nn.Sequential of nn.Linear in float64, the molecule sum by a dense one-hot matrix, gradients by torch.autograd: 1e-12."""
    import torch.nn as nn
    import torch.nn.functional as Fn
    for (n_in, H), N in (((128, 64), 129), ((32, 32), 17), ((128, 160), 333)):
        c = A.make_case(n_in, H, N, name)
        for b1, b2 in ((True, True), (False, True), (True, False), (False, False)):
            l0, l1 = nn.Linear(n_in, H, bias=b1, dtype=torch.float64), nn.Linear(H, 1, bias=b2, dtype=torch.float64)
            with torch.no_grad():
                l0.weight.copy_(c["w1"]); l1.weight.copy_(c["w2"][None, :])
                if b1:
                    l0.bias.copy_(c["b1"])
                if b2:
                    l1.bias.copy_(c["b2"])
            fn = nn.SiLU() if act == "silu" else (lambda v: Fn.softplus(v) - torch.log(torch.tensor(2.0, dtype=torch.float64)))
            onehot = (c["idx_m"][None, :] == torch.arange(c["n_mol"])[:, None]).double()
            for use_gE, use_gy in ((True, True), (True, False), (False, True)):
                x = c["x"].clone().requires_grad_(True)
                pre = l0(x)
                y = l1(fn(pre))[:, 0]
                E = onehot @ y
                (gx,) = torch.autograd.grad((E * c["wE"]).sum() * float(use_gE) + (y * c["wA"]).sum() * float(use_gy), [x])
                ref = A.head_ref(c, act, b1=b1, b2=b2, use_gE=use_gE, use_gy=use_gy)
                figs = {"pre": A.rel(ref["pre"], pre.detach()), "y_atom": A.rel(ref["y_atom"], y.detach()), "E": A.rel(ref["E"], E.detach()),
                        "gx": A.rel(ref["gx"], gx)}
                assert all(v < 1e-12 for v in figs.values()), (c["label"], act, b1, b2, use_gE, use_gy, figs)
                assert (ref["E"][A.empty_ids(c)] == 0).all()


@pytest.mark.parametrize("act", A.ACTS)
def test_float32_on_the_host_stays_below_half_the_device_bound(act):
    """Conditioning of every case of the GPU file (on 256 compute units): the formula in float32 against the formula in float64."""
    worst = {}
    for n_in, H, N, name in A.gpu_cases(N_CU):
        c = A.make_case(n_in, H, N, name)
        ref, f32 = A.head_ref(c, act), A.head_formula(c, act, torch.float32)
        for q in ("pre", "y_atom", "E", "gx"):
            v = A.rel(f32[q], ref[q])
            if v > worst.get(q, (-1.0, ""))[0]:
                worst[q] = (v, c["label"])
            assert v < 0.5 * TOL, (c["label"], act, q, v)
    for q, (v, label) in worst.items():
        print("%-4s float32 on the host, worst %-7s %.2e  (%s)" % (act, q, v, label))
    assert len(A.gpu_cases(N_CU)) >= len(A.FWD16_SHAPES + A.FWD32_SHAPES) * len(A.TILE_NS) * len(A.TILE_LAYOUTS) + 4 * 7 + 8
