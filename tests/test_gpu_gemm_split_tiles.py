"""gemm256w4_split_kernel (csrc/gemm256w4_split.hip) alone: the next-tile hand-off, every raster edge, every epilogue, the K-sliced
form, with operands whose product is exact (tests/gemm_split_ref.py).

To the kernel the operands are a plain f16 GEMM over one walk of 3K columns, out = rs[m] * w_inv * (A16 . W16^T); the tests build
A16 [M, 3K] and W16 [N, 3K] as dense integers in [-3, 3] that differ between the three K segments (split_rows / split_weight are
tested elsewhere), rs and w_inv powers of two, bias and x0 integers.  Every case first asserts (|A16| . |W16|^T).max() < 2^24 on its
own reference: STORE, STORE + bias and RESID_DIV with div = 2 are then exact, and the reference is torch's float64 product of the
same tensors, formed on the device.

Every output is a view into a larger buffer (8 rows above, 256 below, ldc = N + 8 in the odd-M cases and in one hand-off case of
each kind) pre-filled with NaN, or for
RESID_DIV with x0 inside the view and a sentinel outside; the WHOLE buffer is compared (the written region equal to the reference,
everything else still the prefill), and every launch runs twice with identical bits.  Shapes that have to exceed the number of
workgroups come from the device's CU count (256 on an MI355X: the figures in the comments); each hand-off case asserts that it has
more tiles than workgroups (more than twice as many where a tile must both be handed over and hand over).

Not covered, by design: exact operands cannot see a rounding-mode error (test_gemm_split_vs_float64's Gaussian bars keep that);
the 32-bit operand offsets of gemm256w4_tile.inc (an operand of 4 GiB or more) are not run; operand over-reads past row M-1 are
clamped in code and cannot be observed without provoking a fault."""
import ctypes

import pytest
import torch

from tests import gemm_split_ref as gr

pytestmark = pytest.mark.gpu

TOP, SPARE = 8, 256
SENTINEL = 12345.678                      # no exact result: every result is a multiple of 2^-6 (rs * w_inv / 2 >= 2^-6)
NAN = float("nan")
STORE, RESID, SWIGLU = 0, 2, 4


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _tiles(M, N):
    return -(-M // gr.BM) * (N // gr.BN)


class Dev:
    """A case on the device with its float64 product P = A16 . W16^T (integers), the exactness condition asserted."""

    def __init__(self, c: gr.Case):
        self.c = c
        self.A, self.W, self.rs, self.bias = c.A16.cuda(), c.W16.cuda(), c.rs.cuda(), c.bias.cuda()
        gr.assert_exact_inputs(self.A, self.W)
        self.P = self.A.double() @ self.W.double().t()
        assert float((self.P != 0).double().mean()) > 0.9          # the data exercise the kernel

    def v(self, rs=True):
        """float64 rs[m] * w_inv * P."""
        return self.P * ((self.rs.double()[:, None] if rs else 1.0) * self.c.w_inv)


def _same_whole(buf, want, region, tag):
    """Whole-buffer comparison: equal values, NaN where NaN is expected; the report says where the differences are."""
    ok = (buf == want) | (torch.isnan(buf) & torch.isnan(want))
    if bool(ok.all()):
        return
    bad = ~ok
    r0, r1, c1 = region
    inside = int(bad[r0:r1, :c1].sum())
    idx = bad.nonzero()
    i, j = int(idx[0, 0]), int(idx[0, 1])
    raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} elements differ, {inside} inside the written region (rows {r0}.."
                         f"{r1 - 1}, columns 0..{c1 - 1}), {int(bad.sum()) - inside} outside it; {int(torch.isnan(buf[r0:r1, :c1]).sum())} "
                         f"never written; rows {int(idx[:, 0].min())}..{int(idx[:, 0].max())}, columns {int(idx[:, 1].min())}.."
                         f"{int(idx[:, 1].max())}; first at ({i}, {j}): got {float(buf[i, j])}, want {float(want[i, j])}")


def _run(d: Dev, epi, ldc, *, rs=True, bias=False, div=1.0, x0=None):
    """One launch into a fresh prefilled buffer -> the whole buffer [TOP + M + SPARE, ldc]."""
    from esmdiff_amd.engine import gemm_split
    c = d.c
    width = c.N // 2 if epi == SWIGLU else c.N
    buf = torch.full((TOP + c.M + SPARE, ldc), SENTINEL if epi == RESID else NAN, device="cuda")
    if epi == RESID:
        buf[TOP:TOP + c.M, :c.N] = x0
    out = buf[TOP:TOP + c.M]
    assert out.stride(0) == ldc and out.data_ptr() == buf.data_ptr() + TOP * ldc * 4
    got = gemm_split(d.A, d.rs if rs else None, d.W, c.w_inv, width, epi, out=out, bias=d.bias if bias else None, div=div)
    assert got.shape == (c.M, width) and got.data_ptr() == out.data_ptr()
    return buf


def _check(d: Dev, epi, ldc, ref32, tag, **kw):
    """Twice, whole buffer against ref32 [M, N] in the written region and the prefill elsewhere."""
    c = d.c
    first = _run(d, epi, ldc, **kw)
    want = torch.full_like(first, SENTINEL if epi == RESID else NAN)
    want[TOP:TOP + c.M, :c.N] = ref32
    _same_whole(first, want, (TOP, TOP + c.M, c.N), tag)
    assert not bool(torch.isnan(first[TOP:TOP + c.M, :c.N]).any())
    second = _run(d, epi, ldc, **kw)
    assert torch.equal(second.view(torch.int32), first.view(torch.int32)), f"{tag}: second launch differs from the first"
    return first


def _exact_epilogues(d: Dev, ldc, tag, epis=("store", "bias", "resid", "nors")):
    """STORE, STORE + bias, RESID_DIV with div = 2, STORE with rs = NULL: all exact."""
    c = d.c
    if "store" in epis:
        _check(d, STORE, ldc, gr.as_f32_exact(d.v(), "v"), f"{tag} STORE ldc={ldc}")
    if "nors" in epis:
        _check(d, STORE, ldc, gr.as_f32_exact(d.v(rs=False), "v"), f"{tag} STORE rs=NULL ldc={ldc}", rs=False)
    if "bias" in epis:
        _check(d, STORE, ldc, gr.as_f32_exact(d.v() + d.bias.double(), "v + bias"), f"{tag} STORE+bias ldc={ldc}", bias=True)
    if "resid" in epis:
        x0 = c.x0("cuda")
        _check(d, RESID, ldc, gr.as_f32_exact(x0.double() + d.v() / 2, "x0 + v / 2"), f"{tag} RESID_DIV div=2 ldc={ldc}", div=2.0, x0=x0)


def _engine_div(d: Dev, ldc, tag):
    """RESID_DIV with the engine's divisor: bit-equal to the float32 host restatement x0 + v / div (v exact, IEEE division)."""
    c = d.c
    x0 = c.x0("cuda")
    v32 = gr.as_f32_exact(d.v(), "v").cpu()
    want = (x0.cpu() + v32 / torch.tensor(gr.DIV_ENGINE, dtype=torch.float32)).cuda()
    first = _check(d, RESID, ldc, want, f"{tag} RESID_DIV div={gr.DIV_ENGINE} ldc={ldc}", div=gr.DIV_ENGINE, x0=x0)
    assert torch.equal(first[TOP:TOP + c.M, :c.N].contiguous().view(torch.int32), want.view(torch.int32))


def _ldc(M, N):
    return N + 8 if M % 2 else N


# ---- 1. short K loops, one tile and a few tiles ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", gr.SHORT_K)
@pytest.mark.parametrize("N", gr.SHORT_N)
def test_short_k_every_epilogue_exact(N, K):
    """3K / 64 = 6, 12, 18 K-tiles (1, 4, 7 steady iterations); M across the wave-row boundary at 128 and the tile boundary at 256;
    one and three tile columns; every workgroup runs one tile (xnext = 0)."""
    for M in gr.SHORT_M:
        d = Dev(gr.make_case(M, N, K))
        _exact_epilogues(d, _ldc(M, N), f"({M}, {N}, {K})")
        if (M, N, K) == (257, 768, 128):
            _engine_div(d, _ldc(M, N), f"({M}, {N}, {K})")


# ---- 2. raster edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles_m,tiles_n", gr.RASTER, ids=[f"{a}x{b}" for a, b in gr.RASTER])
def test_raster_edges_exact(tiles_m, tiles_n):
    """tiles_m = 4 < GROUP_M; tiles_m = 9: a last group of one tile row; 3 x 3 = 9 tiles: rr = 1 in tile_origin.  K = 128."""
    M, N, K = tiles_m * gr.BM - 3, tiles_n * gr.BN, 128
    assert _tiles(M, N) == tiles_m * tiles_n <= gr.grid_cap(_cus())
    d = Dev(gr.make_case(M, N, K))
    _exact_epilogues(d, _ldc(M, N), f"raster {tiles_m} x {tiles_n}", epis=("store", "resid"))


# ---- 3. / 4. the next-tile hand-off ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["one_round", "one_round_rr"])
def test_hand_off_after_a_six_k_tile_loop_exact(which):
    """17 tile rows (the last ragged) and just more tiles than workgroups (272 or 289 on 256 CUs, the second with rr = 1): every
    workgroup's first tile comes from the prologue, tiles - grid of them take a second one through the hand-off directly after a
    six-K-tile loop (no spare steady iteration); nobody runs a third.  STORE, RESID_DIV with div = 2 and with the engine's."""
    M, N, K = gr.handoff_shapes(_cus())[which]
    tiles, g = _tiles(M, N), gr.grid(_tiles(M, N), _cus())
    assert g < tiles <= 2 * g, f"{tiles} tiles on {g} workgroups: no hand-off, or a third round"
    assert which != "one_round_rr" or tiles % 8 != 0
    d = Dev(gr.make_case(M, N, K))
    _exact_epilogues(d, N + 8 if which == "one_round" else N, f"hand-off {tiles} tiles / {g}", epis=("store", "resid"))
    if which == "one_round":
        _engine_div(d, N, f"hand-off {tiles} tiles / {g}")


@pytest.mark.parametrize("which", ["two_rounds", "two_rounds_k256"])
def test_hand_off_chained_exact(which):
    """33 tile rows and more than twice as many tiles as workgroups (528 on 256 CUs): a tile that was handed over and hands over
    (have_k0 and xnext together); at K = 256 with four steady iterations in between.  Compared on the device (138 MB)."""
    M, N, K = gr.handoff_shapes(_cus())[which]
    tiles, g = _tiles(M, N), gr.grid(_tiles(M, N), _cus())
    assert tiles > 2 * g, f"{tiles} tiles on {g} workgroups: no workgroup runs three"
    d = Dev(gr.make_case(M, N, K))
    _exact_epilogues(d, N + 8 if which == "two_rounds" else N, f"chained hand-off {tiles} tiles / {g}",
                     epis=("store", "resid") if which == "two_rounds" else ("store",))


# ---- 5. the fused SwiGLU (launcher code 4) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(4), ids=["M1", "M129", "M257", "hand_off"])
def test_swiglu_epilogue_vs_float64(i):
    """W rows interleaved by the host restatement; out f32 [M, N / 2] against g sigmoid(g) u in float64 within
    COEF(g) 2^-24 |ref| + 2^-24 |u|; gates below -88.7 (exp2 overflows: the kernel gives 0), above 20 and exactly 0 included.
    Columns N / 2 .. ldc-1 and every row outside the view stay NaN."""
    M, N, K = gr.swiglu_shapes(_cus())[i]
    if i == 3:
        tiles, g = _tiles(M, N), gr.grid(_tiles(M, N), _cus())
        assert g < tiles <= 2 * g
    c = gr.make_swiglu_case(M, N, K)
    d = Dev(c)
    gate, up = gr.deinterleave_columns(d.v())
    gr.assert_gate_span(gate)
    ref, t, floor = gr.swiglu_ref64(gate, up)
    FH = N // 2
    ldc = FH + 8 if i != 2 else FH
    first = _run(d, SWIGLU, ldc)
    second = _run(d, SWIGLU, ldc)
    got = first[TOP:TOP + M, :FH]
    c0, c1 = gr.swiglu_needed(got, gate, up)
    total = gr.swiglu_needed_total(got, gate, up)
    # measured on an MI355X: c0 1.60, 2.47, 2.63, 2.76, c1 0.80, 0.81, 0.80, 0.83 (the float32 emulation's figures), 0.089 - 0.165 of the bar
    print(f"MEASURED split GEMM epilogue 4 ({M}, {N}, {K}): c0 {c0:.2f} of {gr.SWIGLU4_C0:g}, c1 {c1:.2f} of {gr.SWIGLU4_C1:g}, "
          f"largest error {total:.3f} of the bar")
    assert not bool(torch.isnan(got).any()), f"{int(torch.isnan(got).sum())} elements never written"
    outside = torch.ones_like(first, dtype=torch.bool)
    outside[TOP:TOP + M, :FH] = False
    assert bool(torch.isnan(first[outside]).all()), "a store outside [M, N / 2]"
    err = (got.double() - ref).abs()
    bad = err > gr.swiglu_bar(ref, t, floor)
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[0].tolist(), total)
    assert bool((got[gate < -88.8] == 0).all())
    assert torch.equal(second.view(torch.int32), first.view(torch.int32)), "second launch differs from the first"


# ---- 7. the K-sliced form ------------------------------------------------------------------------------------------------------------
def _kslice(M, N, K, S, tag):
    """parts[s, :M] = w_inv * (slice s of A16) . (slice s of W16)^T exactly, rs NOT applied; x = x0 + sum * rs / div exactly for
    div = 2, bit-equal to the float32 restatement for the engine's div.  Rows M .. m_pad-1 of each plane are unspecified (the
    kernel writes products of the clamped last row there) and not asserted; nothing outside [S, m_pad, N] is written."""
    from esmdiff_amd.engine import gemm_split_k
    c = gr.make_case(M, N, K)
    A, W, rs = c.A16.cuda(), c.W16.cuda(), c.rs.cuda()
    gr.assert_exact_inputs(A, W)
    ks = 3 * K // S
    P = torch.stack([A[:, s * ks:(s + 1) * ks].double() @ W[:, s * ks:(s + 1) * ks].double().t() for s in range(S)])
    assert all(not torch.equal(P[0], P[s]) for s in range(1, S))
    want_parts = gr.as_f32_exact(P * c.w_inv, "slice products")
    m_pad = -(-M // 256) * 256
    pad, n = SPARE * N, S * m_pad * N
    x0 = c.x0("cuda")
    v = P.sum(0) * (rs.double()[:, None] * c.w_inv)
    v32 = gr.as_f32_exact(v, "v")
    wants = {2.0: gr.as_f32_exact(x0.double() + v / 2, "x0 + v / 2"),
             gr.DIV_ENGINE: (x0.cpu() + v32.cpu() / torch.tensor(gr.DIV_ENGINE, dtype=torch.float32)).cuda()}
    for div, want_x in wants.items():
        bits = None
        for _ in range(2):
            flat = torch.full((pad + n + pad,), NAN, device="cuda")
            parts = flat[pad:pad + n].view(S, m_pad, N)
            xbuf = torch.full((TOP + M + SPARE, N), SENTINEL, device="cuda")
            xbuf[TOP:TOP + M] = x0
            ret = gemm_split_k(A, rs, W, c.w_inv, xbuf[TOP:TOP + M], S, div=div, parts=parts)
            assert ret.data_ptr() == parts.data_ptr()
            assert bool(torch.isnan(flat[:pad]).all()) and bool(torch.isnan(flat[pad + n:]).all()), f"{tag}: a store outside parts"
            got = parts[:, :M]
            assert not bool(torch.isnan(got).any()), f"{tag}: {int(torch.isnan(got).sum())} elements of parts never written"
            if not torch.equal(got, want_parts):
                bad = (got != want_parts).nonzero()
                s, i, j = bad[0].tolist()
                raise AssertionError(f"{tag}: {bad.shape[0]} of {got.numel()} elements of parts differ, planes {int(bad[:, 0].min())}.."
                                     f"{int(bad[:, 0].max())}, rows {int(bad[:, 1].min())}..{int(bad[:, 1].max())}; first at ({s}, {i}, {j}): "
                                     f"got {float(got[s, i, j])}, want {float(want_parts[s, i, j])}")
            wx = torch.full_like(xbuf, SENTINEL)
            wx[TOP:TOP + M] = want_x
            _same_whole(xbuf, wx, (TOP, TOP + M, N), f"{tag} x, div={div}")
            assert torch.equal(xbuf[TOP:TOP + M].view(torch.int32), want_x.view(torch.int32))
            now = (got.contiguous().view(torch.int32).clone(), xbuf.view(torch.int32).clone())
            assert bits is None or (torch.equal(bits[0], now[0]) and torch.equal(bits[1], now[1])), f"{tag}: second launch differs"
            bits = now


@pytest.mark.parametrize("S,K", gr.KSLICE_SK, ids=[f"S{s}_K{k}" for s, k in gr.KSLICE_SK])
def test_k_slices_of_6_8_10_k_tiles_exact(S, K):
    assert gr.kslice_tiles(S, K) in (6, 8, 10)
    for N in gr.KSLICE_N:
        for M in gr.KSLICE_M:
            _kslice(M, N, K, S, f"K-sliced S={S} ({M}, {N}, {K})")


def test_k_sliced_hand_off_across_slice_boundaries_exact():
    """S = 4 slices of five tile rows: 20 virtual tile rows x 16 columns = 320 virtual tiles on 256 CUs; the groups of 8 virtual
    tile rows straddle the slice boundaries at 5, 10, 15, and 64 workgroups are handed a second tile, some in another slice."""
    S, M, N, K = gr.kslice_handoff_shape(_cus())
    tiles = S * _tiles(M, N)
    g = gr.grid(tiles, _cus())
    assert g < tiles <= 2 * g and (5 % gr.GROUP_M, 10 % gr.GROUP_M, 15 % gr.GROUP_M) != (0, 0, 0)
    # some workgroup's two tiles lie in different slices (the raster restated): the hand-off then changes the source columns too
    assert any(gr.tile_origin(vt, 20, N // 256)[0] // 5 != gr.tile_origin(vt + g, 20, N // 256)[0] // 5 for vt in range(tiles - g))
    _kslice(M, N, K, S, f"K-sliced hand-off S={S} ({M}, {N}, {K}), {tiles} virtual tiles / {g}")


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
REFUSED = [
    # M, N, K, ldc, epilogue, why
    (200, 384, 128, 384, STORE, "N % 256 != 0"),
    (200, 256, 192, 256, STORE, "K % 128 != 0"),
    (200, 512, 128, 508, STORE, "ldc < N"),
    (200, 256, 128, 258, STORE, "ldc % 4 != 0"),
    (200, 512, 128, 252, SWIGLU, "epilogue 4 with ldc < N / 2"),
    (200, 256, 128, 256, 1, "BIAS_GELU is not an epilogue of the split GEMM"),
    (200, 256, 128, 256, 3, "the launcher's own code for STORE with a bias is not accepted from outside"),
    (200, 256, 128, 256, 5, "an unknown epilogue"),
]


@pytest.mark.parametrize("M,N,K,ldc,epi,why", REFUSED, ids=[w.replace(" ", "_") for *_, w in REFUSED])
def test_refused_before_any_launch(M, N, K, ldc, epi, why):
    """Refused by the launcher itself (the entry is called directly: the Python wrapper would assert first): an error, and the
    sentinel-filled output is untouched."""
    from esmdiff_amd import _native as Nn
    A = torch.ones(M, 3 * K, dtype=torch.float16, device="cuda")
    W = torch.ones(N, 3 * K, dtype=torch.float16, device="cuda")
    bias = torch.zeros(N, device="cuda")
    out = torch.full((M + SPARE, max(ldc, N)), 3.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                     # noqa: E731
    with pytest.raises(RuntimeError, match="libesmdiff_hip error"):
        Nn.check(Nn.lib().esmdiff_gemm_split(p(A), None, p(W), 1.0, p(out), p(bias), M, N, K, ldc, 1.0, epi,
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()), why
