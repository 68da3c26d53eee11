"""What tests/test_gpu_gemm_split_tiles.py relies on, checked without a GPU (tests/gemm_split_ref.py): the exactness condition on
every case it runs, the shape helper that makes the next-tile hand-off happen, the host restatement of the gate / up row interleave,
and the SwiGLU bar: the float32 emulation of the kernel's expression is inside it, its two constants are 4 x what that emulation
needs, and two wrong results leave it."""
import math

import pytest
import torch

from tests import gemm_split_ref as gr

CUS = (256, 304)


def _pow2_ceil(x: float) -> float:
    return 2.0 ** math.ceil(math.log2(x))


def test_every_case_of_the_gpu_file_is_exact():
    """(|A16| . |W16|^T).max() < 2^24 on the tensors the GPU file runs, operands are dense integers in [-3, 3] that differ between
    the three K segments, scales are powers of two."""
    seen = set()
    for cus in CUS:
        shapes = [(s, gr.make_case) for s in gr.all_exact_shapes(cus)] + [(s, gr.make_swiglu_case) for s in gr.swiglu_shapes(cus)]
        for (M, N, K), make in shapes:
            if (M, N, K, make) in seen:
                continue
            seen.add((M, N, K, make))
            c = make(M, N, K)
            # the bound holds for every draw (9 * 3K); the product itself is formed where it is cheap, the row sums elsewhere
            assert 9 * 3 * K < 2 ** 24
            if M * N * K <= 2 ** 31:
                gr.assert_exact_inputs(c.A16, c.W16)
            else:
                assert float(c.A16.float().abs().sum(1).max()) * float(c.W16.float().abs().max()) < 2 ** 24
            for X in (c.A16, c.W16):
                x = X.float()
                assert float(x.abs().max()) == 3 and bool((x == x.round()).all())
                assert float((x != 0).float().mean()) > 0.8                                    # dense: 6 of 7 values
                segs = x.view(X.shape[0], 3, K)
                assert not torch.equal(segs[:, 0], segs[:, 1]) and not torch.equal(segs[:, 0], segs[:, 2]) and not torch.equal(segs[:, 1], segs[:, 2])
            e = torch.log2(c.rs)
            assert bool((e == e.round()).all()) and float(e.min()) >= -3 and float(e.max()) <= 3
            assert math.log2(c.w_inv) == round(math.log2(c.w_inv))
    assert len(seen) > 60


def test_exact_epilogues_are_float32_numbers():
    """STORE, bias, RESID_DIV with div = 2 and the K-slice planes of a short and a long K are exact in float32 (the condition
    as_f32_exact asserts in the GPU file), by the worst case of the generator: |sum| <= 9 * 3K, scales 2^-3 .. 2^3 * w_inv / 2."""
    for K in (128, 640):
        worst = 9 * 3 * K * 8 * 0.25 + 8 + 8           # the largest |value|: sum * rs * w_inv + bias or x0
        step = 2.0 ** -3 * 0.25 / 2                   # the smallest spacing: rs * w_inv / div
        assert worst / step < 2 ** 24
    c = gr.make_case(257, 256, 128)
    v = (c.A16.double() @ c.W16.double().t()) * (c.rs.double()[:, None] * c.w_inv)
    gr.as_f32_exact(v, "v")
    gr.as_f32_exact(v + c.bias.double(), "v + bias")
    gr.as_f32_exact(c.x0().double() + v / 2, "x0 + v / 2")
    with pytest.raises(AssertionError, match="not exact"):
        gr.as_f32_exact(v / 3, "v / 3")


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_shape_helper_makes_the_hand_off_happen(cus):
    cap = gr.grid_cap(cus)
    assert cap == cus // 8 * 8 and gr.grid(5, cus) == 5 and gr.grid(10 ** 6, cus) == cap
    for tiles_m in (17, 20, 33):
        tn = gr.tiles_n_for_rounds(tiles_m, 1, cus)
        assert tiles_m * tn > cap >= tiles_m * (tn - 1)                     # more tiles than workgroups, and the smallest such
        tr = gr.tiles_n_ragged(tiles_m, 1, cus)
        assert tr > tn and tiles_m * tr % 8 != 0
    if cus == 64:
        return
    tn2 = gr.tiles_n_for_rounds(33, 2, cus)
    assert 33 * tn2 > 2 * cap >= 33 * (tn2 - 1)
    hs = gr.handoff_shapes(cus)
    for tag, rounds in (("one_round", 1), ("one_round_rr", 1), ("two_rounds", 2), ("two_rounds_k256", 2)):
        M, N, K = hs[tag]
        tiles = -(-M // 256) * (N // 256)
        g = gr.grid(tiles, cus)
        assert rounds * g < tiles <= (rounds + 1) * g, (tag, tiles, g)
        assert M % 256 != 0                                                  # a ragged last tile row
    assert (-(-hs["one_round_rr"][0] // 256) * (hs["one_round_rr"][1] // 256)) % 8 != 0
    S, M, N, K = gr.kslice_handoff_shape(cus)
    tiles = S * -(-M // 256) * (N // 256)
    assert gr.grid(tiles, cus) < tiles and (S * -(-M // 256)) % 8 != 0 and -(-M // 256) % 8 != 0
    if cus == 256:                                                           # the shapes the issue names
        assert hs == {"one_round": (4252, 4096, 128), "one_round_rr": (4252, 4352, 128), "two_rounds": (8348, 4096, 128),
                      "two_rounds_k256": (8348, 4096, 256)}
        assert (S, M, N, K) == (4, 1180, 4096, 512) and tiles == 320


@pytest.mark.parametrize("tiles_m,tiles_n", [(4, 3), (9, 3), (3, 3), (17, 16), (17, 17), (33, 16), (20, 16), (1, 1), (2, 3)])
def test_raster_restatement_visits_every_tile_once(tiles_m, tiles_n):
    """tile_origin as restated here is a bijection (what the raster must be for every tile to be written once), and the K-sliced
    hand-off case has groups of 8 virtual tile rows that straddle a slice boundary."""
    seen = {gr.tile_origin(vt, tiles_m, tiles_n) for vt in range(tiles_m * tiles_n)}
    assert seen == {(r, c) for r in range(tiles_m) for c in range(tiles_n)}
    if (tiles_m, tiles_n) == (20, 16):
        assert all(boundary % gr.GROUP_M != 0 for boundary in (5, 10, 15))     # every slice boundary lies inside a group of 8


def test_interleave_restatement_round_trips():
    g = torch.Generator().manual_seed(3)
    Wg, Wu = torch.randn(96, 24, generator=g), torch.randn(96, 24, generator=g)
    W = gr.interleave_swiglu(Wg, Wu)
    assert W.shape == (192, 24)
    assert torch.equal(W[:32], Wg[:32]) and torch.equal(W[32:64], Wu[:32]) and torch.equal(W[64:96], Wg[32:64])
    assert torch.equal(W[128 + 32 + 7], Wu[64 + 7])
    g2, u2 = gr.deinterleave_swiglu(W)
    assert torch.equal(g2, Wg) and torch.equal(u2, Wu)
    A = torch.randn(5, 24, generator=g)
    pg, pu = gr.deinterleave_columns(A @ W.t())
    assert torch.equal(pg, A @ Wg.t()) and torch.equal(pu, A @ Wu.t())


def _swiglu_grids(cus=256):
    for M, N, K in gr.swiglu_shapes(cus):
        c = gr.make_swiglu_case(M, N, K)
        g, u = gr.swiglu_gates_ups(c)
        yield (M, N, K), g, u


def test_swiglu_bar_holds_the_float32_emulation_and_its_constants_are_measured():
    c0 = c1 = 0.0
    flat_fails = False
    for shape, g, u in _swiglu_grids():
        gr.assert_gate_span(g)
        g32, u32 = gr.as_f32_exact(g, "gate"), gr.as_f32_exact(u, "up")      # rs * w_inv * integer: what the kernel holds
        emu = gr.swiglu4_emulation(g32, u32)
        assert bool(torch.isfinite(emu).all()), shape
        ref, t, floor = gr.swiglu_ref64(g, u)
        assert bool(((emu.double() - ref).abs() <= gr.swiglu_bar(ref, t, floor)).all()), shape
        assert bool((emu[g < -88.8] == 0).all())                              # exp2 overflowed: the floor's case
        # without the floor the flat coefficient alone does not hold the negative side: the derived term is what does
        rel = (emu.double() - ref).abs() - gr.F32_EPS * ref.abs() * (gr.SWIGLU4_C0 + gr.SWIGLU4_C1 * t)
        sel = (g >= gr.SWIGLU4_MEASURE_G_MIN) & (ref != 0)
        assert float(rel[sel].max()) <= 0
        flat_fails = flat_fails or bool(((emu.double() - ref).abs() > gr.F32_EPS * ref.abs() * gr.SWIGLU4_C0)[sel].any())
        a, b = gr.swiglu_needed(emu, g, u)
        print(f"MEASURED float32 emulation of epilogue 4 at {shape}: c0 {a:.2f}, c1 {b:.2f}")
        c0, c1 = max(c0, a), max(c1, b)
    print(f"MEASURED float32 emulation of epilogue 4: c0 {c0:.2f} -> {_pow2_ceil(4 * c0):g}, c1 {c1:.2f} -> {_pow2_ceil(4 * c1):g}")
    assert 4 * c0 <= gr.SWIGLU4_C0 <= 16 * c0, c0
    assert 4 * c1 <= gr.SWIGLU4_C1 <= 16 * c1, c1
    assert flat_fails
    # ... and with the floor it never binds: t |g sigmoid(g)| <= 0.64, i.e. at most 0.64 * 2^-24 |u| per unit of c1
    gg = torch.linspace(-200, 200, 400001, dtype=torch.float64)
    _, tt, _ = gr.swiglu_ref64(gg, torch.ones_like(gg))
    assert 0.63 < float((tt * (gg * torch.sigmoid(gg)).abs()).max()) < 0.64


def test_swiglu_bar_can_fail():
    """Gate and up swapped; one 32-row block of W not interleaved (its gate and up columns come out as the plain rows would)."""
    M, N, K = 129, 512, 128
    c = gr.make_swiglu_case(M, N, K)
    g, u = gr.swiglu_gates_ups(c)
    ref, t, floor = gr.swiglu_ref64(g, u)
    bar = gr.swiglu_bar(ref, t, floor)
    swapped = gr.swiglu4_emulation(u.float(), g.float())
    assert not bool(((swapped.double() - ref).abs() <= bar).all())
    # block 1 (interleaved rows 64 .. 127) laid out as plain rows [gate 32 .. 63 | gate 64 .. 95] instead of [gate 32 .. 63 | up 32 .. 63]
    Wg, Wu = gr.deinterleave_swiglu(c.W16)
    Wbad = c.W16.clone()
    Wbad[96:128] = Wg[64:96]
    P = (c.A16.double() @ Wbad.double().t()) * (c.rs.double()[:, None] * c.w_inv)
    gb, ub = gr.deinterleave_columns(P)
    bad = gr.swiglu4_emulation(gb.float(), ub.float())
    out = (bad.double() - ref).abs() > bar
    assert bool(out.any()) and not bool(out[:, :32].any()) and not bool(out[:, 64:].any())     # that block, and only it
