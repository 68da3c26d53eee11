"""The 16-bit GEMMs at every boundary of their dispatcher (csrc/gemm.hip: choose_gemm), with operands whose product is exact.

Every case first asserts, through esmdiff_describe_gemm_choice (answered by the dispatcher the launcher itself calls), that its
shape runs on the code path it was written for: the four-wave 256x256 kernel, the 128-column kernel with 64- or 128-row tiles and
four or two LDS stages, its split-K form, or the raw K-slice planes the add+LayerNorm kernel sums.  A retuned threshold then fails
the case with "this shape no longer runs on the path it was written for" instead of silently testing something else.

Exact operands: A and W entries are a random sign times a Bernoulli(min(1, 8 / sqrt(K))) mask, so every product and every f32
partial sum is an integer (standard deviation 8), exact whatever the K order or slicing; with alpha = 0.5 the result is exact in
bf16 and f16 as long as |sum| <= 128, which each test asserts on its float64 reference (a condition on the inputs, not a
tolerance).  Comparisons of EPI_BF16, EPI_RESID_F32 and EPI_BIAS_F32 are therefore torch.equal on the whole output buffer,
pre-filled with NaN (16-bit) or a sentinel (f32 stores) so that an unwritten tile fails; every launch runs twice and the second
result must equal the first bit for bit.  The same data goes through the bf16 and the f16 build.

EPI_SWIGLU_BF16 and EPI_BIAS_GELU_BF16 go through v_rcp / exp2 / erff and are not exact: they run at the same shapes with the
Gaussian operands and the float64 bars of tests/test_gpu_gemm_mfma16.py (split-K: of test_gemm_small_m_split_k).

EPI_BIAS_F32 pins what both kernels do with n_valid (include/esmdiff_hip_test.h): a 4-column group is skipped only when it would
cross ldc, so columns n_valid .. ldc-1 receive the bias (their weight rows are zero)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [(BF16, "bf16"), (F16, "f16")]
SENTINEL = 12345.678                      # no exact result is a non-integer multiple of 0.5 this large
SMALL_MAX_ROWS = 1152                     # small_max_rows()

# the dispatcher's answer: the 256x256 kernel (its own two 64 KiB stages), or the 128-column kernel with rows / K slices / stages
W4 = {"w4": True, "rows": 256, "S": 1, "stages": 2}


def T(rows, stages, S=1):
    return {"w4": False, "rows": rows, "S": S, "stages": stages}


def _choice(M, N, K, ws_floats=0):
    from esmdiff_amd import _native as Nn
    return Nn.gemm_choice(M, N, K, ws_floats)


def _assert_choice(M, N, K, want, ws_floats=0):
    got = _choice(M, N, K, ws_floats)
    assert got == want, f"({M}, {N}, {K}) no longer runs on the path it was written for: dispatcher {got}, case {want}"


def _fn(dt, eng=None):
    from esmdiff_amd.engine import gemm_bf16, gemm_f16
    if eng is not None:
        assert dt == BF16
        return eng.gemm
    return gemm_bf16 if dt == BF16 else gemm_f16


def _seed(M, N, K):
    return (1000003 * M + 1009 * N + K) % (2 ** 31 - 1)


def _exact_operands(M, N, K):
    """A [M,K], W [N,K] f32 with entries in {-1, 0, +1}, x0 [M,N] and bias [N] small integers, ref = A W^T in float64."""
    g = torch.Generator(device="cuda").manual_seed(_seed(M, N, K))
    p = min(1.0, 8.0 / K ** 0.5)

    def tern(r, c):
        sign = torch.randint(0, 2, (r, c), generator=g, device="cuda", dtype=torch.int8) * 2 - 1
        return (sign * (torch.rand(r, c, generator=g, device="cuda") < p)).float()
    A, W = tern(M, K), tern(N, K)
    x0 = torch.randint(-8, 9, (M, N), generator=g, device="cuda").float()
    bias = torch.randint(-8, 9, (N,), generator=g, device="cuda").float()
    ref = A.double() @ W.double().t()
    assert float(ref.abs().max()) <= 128, "inputs: |A W^T| must stay <= 128 for 0.5 * sum to be exact in bf16; choose another seed"
    assert float((ref != 0).double().mean()) > 0.5      # the data exercise the kernel: most outputs are non-zero
    return A, W, x0, bias, ref


def _same(out, want, tag):
    """torch.equal with a report: how many elements differ (NaN = never written) and where."""
    assert out.shape == want.shape and out.dtype == want.dtype, (tag, out.shape, want.shape, out.dtype, want.dtype)
    if torch.equal(out, want):
        return
    bad = (out != want) | (out != out)
    idx = bad.nonzero()
    rows, cols = idx[:, 0], idx[:, 1]
    unwritten = int(((out != out) | (out == SENTINEL)).sum())
    i, j = int(rows[0]), int(cols[0])
    raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} elements differ ({unwritten} never written), rows "
                         f"{int(rows.min())}..{int(rows.max())}, columns {int(cols.min())}..{int(cols.max())}; first at ({i}, {j}): "
                         f"got {float(out[i, j])}, want {float(want[i, j])}")


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _twice(launch, want, tag):
    first = launch()
    _same(first, want, tag)
    second = launch()
    assert torch.equal(_bits(second), _bits(first)), f"{tag}: second launch differs from the first"


def _bias_layout(N):
    """n_valid = N - 251 (4101 of 4352, the structure head's ragged tail), ldc = n_valid rounded up to 4; a one-tile N keeps the
    same form: the last 4-column groups cross ldc."""
    nv = N - 251 if N > 256 else N - 7
    return nv, (nv + 3) // 4 * 4


def _check_exact(fn, dt, ops, epis, tag):
    """The exact epilogues of one (kernel build, shape) on the operands of _exact_operands."""
    from esmdiff_amd import _native as Nn
    A32, W32, x0, bias, ref = ops
    M, N = ref.shape
    A, W = A32.to(dt), W32.to(dt)
    if "store" in epis:
        def launch():
            o = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
            fn(A, W, Nn.EPI_BF16, out=o, alpha=0.5)
            return o
        _twice(launch, (ref * 0.5).to(dt), f"{tag} EPI_BF16")
    if "resid" in epis:
        def launch():
            x = x0.clone()
            fn(A, W, Nn.EPI_RESID_F32, out=x, alpha=0.5)
            return x
        _twice(launch, (x0.double() + ref * 0.5).float(), f"{tag} EPI_RESID_F32")
    if "bias" in epis:
        nv, ldc = _bias_layout(N)
        Wp = W.clone()
        Wp[nv:] = 0                                     # the padded weight rows, as the engine loads them
        refp = ref.clone()
        refp[:, nv:] = 0

        def launch():
            o = torch.full((M, ldc), SENTINEL, device="cuda")
            fn(A, Wp, Nn.EPI_BIAS_F32, out=o, bias=bias, n_valid=nv)
            return o
        # columns < n_valid: ref + bias; n_valid .. ldc-1: the bias; a write past ldc would land in the next row
        _twice(launch, (refp + bias.double())[:, :ldc].float().contiguous(), f"{tag} EPI_BIAS_F32 n_valid={nv} ldc={ldc}")


def _gauss_operands(M, N, K, dt, seed=None):
    """The operands of tests/test_gpu_gemm_mfma16.py: A ~ N(0, 1), W ~ N(0, 1 / K), rounded to the 16-bit type."""
    g = torch.Generator(device="cuda").manual_seed(_seed(M, N, K) if seed is None else seed)
    A = torch.randn(M, K, generator=g, device="cuda").to(dt)
    W = (torch.randn(N, K, generator=g, device="cuda") / K ** 0.5).to(dt)
    bias = torch.randn(N, generator=g, device="cuda")
    return A, W, bias


def _check_store_gauss(out, ref, dt, alpha, tag):
    """EPI_BF16 on Gaussian operands: the bar of test_w4_epilogues_vs_float64 (one 16-bit rounding + accumulation noise)."""
    f16 = dt == F16
    e = (out.double() - ref * alpha).abs()
    assert float((e - ref.abs() * alpha * (2 ** -11 if f16 else 2 ** -8)).max()) < (5e-4 if f16 else 4e-3), (tag, float(e.max()))


def _check_inexact(fn, dt, M, N, K, epis, tag, splitk=False):
    """EPI_SWIGLU_BF16 / EPI_BIAS_GELU_BF16 against float64 by the bars of test_w4_epilogues_vs_float64; GELU through split-K by
    the bar of test_gemm_small_m_split_k."""
    from esmdiff_amd import _native as Nn
    if not ({"swiglu", "gelu"} & set(epis)):
        return
    A, W, bias = _gauss_operands(M, N, K, dt)
    ref = A.double() @ W.double().t()
    f16 = dt == F16
    if "swiglu" in epis:
        out = fn(A, W, Nn.EPI_SWIGLU_BF16)
        r = ref.view(M, N // 64, 2, 32)
        want = (torch.nn.functional.silu(r[:, :, 0]) * r[:, :, 1]).reshape(M, N // 2)
        e = (out.double() - want).abs()
        assert out.shape == (M, N // 2) and out.dtype == dt
        assert float((e - want.abs() * (2 ** -10 if f16 else 2 ** -7)).max()) < (1.5e-3 if f16 else 1e-2), (tag, float(e.max()))
        assert torch.equal(_bits(fn(A, W, Nn.EPI_SWIGLU_BF16)), _bits(out)), f"{tag} swiglu: second launch differs"
    if "gelu" in epis:
        out = fn(A, W, Nn.EPI_BIAS_GELU_BF16, bias=bias)
        want = torch.nn.functional.gelu(ref + bias.double())
        e = (out.double() - want).abs()
        if splitk:
            assert float(e.max()) < 3e-2 and float(e.mean()) < 2e-3, (tag, float(e.max()), float(e.mean()))
        elif f16:
            assert float(e.max()) < 4e-3 and float(e.mean()) < 3e-4, (tag, float(e.max()), float(e.mean()))
        else:
            assert float((e - want.abs() * 2 ** -7).max()) < 1e-2 and float(e.mean()) < 2e-3, (tag, float(e.max()), float(e.mean()))
        assert torch.equal(_bits(fn(A, W, Nn.EPI_BIAS_GELU_BF16, bias=bias)), _bits(out)), f"{tag} gelu: second launch differs"


def _cu_columns():
    """256 * (grid // 12 + 3) columns, grid = the CU count rounded down to a multiple of 8 as in persistent_grid(): with 12 row
    tiles that is 36 tiles more than workgroups (6144 columns, 288 tiles on 256 CUs), so some workgroups run two tiles, some one."""
    grid = torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8
    return 256 * (grid // 12 + 3)


# ---- the 256x256 kernel at its shortest K loops -------------------------------------------------------------------------------
ALL5 = ("store", "resid", "bias", "swiglu", "gelu")
W4_CASES = [
    # (M, N, K), epilogues, expected choice, why the shape is here
    ((2817, 1536, 384), ALL5, W4, "12 x 6 = 72 tiles, the fewest admitted; nk = 6: the steady loop runs once; the last row tile "
                                  "holds one row; fewer tiles than CUs: no workgroup has a next tile"),
    ((2817, 1536, 512), ("store",), W4, "nk = 8: two steady iterations"),
    ((2817, 1536, 640), ("store",), W4, "nk = 10: three steady iterations"),
    ((769, 8192, 384), ("store", "swiglu"), W4, "tiles_m = 4 < GROUP_M: one ragged tile-row group, 128 tiles, M below the "
                                                "small-batch switch (FFN-up at ~1 000 rows)"),
    ((2817, "cu", 384), ("store", "resid"), W4, "more tiles than CUs by 36: have_k0 and the next-tile stream right after a "
                                                "six-K-tile loop, beside workgroups with one tile"),
    ((2817, 4352, 384), ("bias",), W4, "n_valid = 4101, ldc = 4104: the ragged head at the shortest K"),
]


@pytest.mark.parametrize("shape,epis,want,why", W4_CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s, *_ in W4_CASES])
def test_w4_short_k_exact(shape, epis, want, why):
    M, N, K = shape
    if N == "cu":
        N = _cu_columns()
        grid = torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8
        assert grid < 12 * (N // 256) < 2 * grid          # some workgroups run two tiles, some one, none three
    _assert_choice(M, N, K, want)
    ops = _exact_operands(M, N, K)
    for dt, name in DTYPES:
        _check_exact(_fn(dt), dt, ops, epis, f"{name} ({M}, {N}, {K})")
    del ops
    for dt, name in DTYPES:
        _check_inexact(_fn(dt), dt, M, N, K, epis, f"{name} ({M}, {N}, {K})")


# ---- neighbours across every dispatch threshold ---------------------------------------------------------------------------------
THRESHOLDS = [
    # (M below, M above, N, K), choice below, choice above, which threshold
    ((2816, 2817, 1536, 384), T(128, 2), W4, "t256 >= 72 && t256m >= 12: 66 tiles of the 128-column kernel against 72 of the 256x256"),
    ((1151, 1152, 1536, 192), T(64, 4), T(128, 4), "small_max_rows()"),
    ((384, 385, 4608, 320), T(64, 4), T(128, 4), "small_tile_mi(): 3 x 36 = 108 <= 128 < 4 x 36 = 144 tiles of 128 rows"),
    ((2688, 2689, 1536, 192), T(128, 4), T(128, 2), "tiles * S <= 256: 21 x 12 = 252 against 22 x 12 = 264, four stages against two"),
    ((2560, 2561, 3072, 384), T(128, 2), W4, "t256 >= 128 below twelve tile rows: 10 x 12 = 120 tiles against 11 x 12 = 132"),
]


@pytest.mark.parametrize("shape,below,above,why", THRESHOLDS, ids=[f"{s[0]}|{s[1]}x{s[2]}x{s[3]}" for s, *_ in THRESHOLDS])
def test_rows_do_not_depend_on_the_side_of_a_threshold(shape, below, above, why):
    """A sample's logits do not depend on the batch it is in: the same A rows inside two batches on either side of a dispatch
    threshold give the same bits (Gaussian operands: with the exact ones the equality would be trivial), and both sides meet the
    float64 bar of test_w4_epilogues_vs_float64."""
    from esmdiff_amd import _native as Nn
    m_lo, m_hi, N, K = shape
    _assert_choice(m_lo, N, K, below)
    _assert_choice(m_hi, N, K, above)
    for dt, name in DTYPES:
        A, W, _ = _gauss_operands(m_hi, N, K, dt)
        ref = A.double() @ W.double().t()
        fn = _fn(dt)
        hi = fn(A, W, Nn.EPI_BF16, alpha=0.866)
        lo = fn(A[:m_lo].contiguous(), W, Nn.EPI_BF16, alpha=0.866)
        _check_store_gauss(hi, ref, dt, 0.866, f"{name} M = {m_hi}")
        _check_store_gauss(lo, ref[:m_lo], dt, 0.866, f"{name} M = {m_lo}")
        _same(_bits(lo), _bits(hi[:m_lo].contiguous()), f"{name} rows 0..{m_lo - 1} of M = {m_lo} against M = {m_hi} ({why})")
        g = torch.Generator(device="cuda").manual_seed(K)
        x0 = torch.randn(m_hi, N, generator=g, device="cuda")
        xh, xl = x0.clone(), x0[:m_lo].clone()
        fn(A, W, Nn.EPI_RESID_F32, out=xh, alpha=0.5)
        fn(A[:m_lo].contiguous(), W, Nn.EPI_RESID_F32, out=xl, alpha=0.5)
        assert float((xh.double() - (x0.double() + ref * 0.5)).abs().max()) < 1e-3
        _same(_bits(xl), _bits(xh[:m_lo].contiguous()), f"{name} EPI_RESID_F32 rows of M = {m_lo} against M = {m_hi} ({why})")


@pytest.mark.parametrize("K", [320, 256])
def test_k_the_256_kernel_does_not_admit_stays_on_the_128_column_kernel(K):
    """M = 2817, N = 1536 has the 72 tiles of the 256x256 kernel, but K = 320 is no multiple of 128 and K = 256 is fewer than six
    K-tiles: the 128-column kernel, two stages (23 x 12 = 276 tiles).  Exact, and Gaussian against float64."""
    from esmdiff_amd import _native as Nn
    M, N = 2817, 1536
    _assert_choice(M, N, K, T(128, 2))
    ops = _exact_operands(M, N, K)
    for dt, name in DTYPES:
        _check_exact(_fn(dt), dt, ops, ("store", "resid"), f"{name} ({M}, {N}, {K})")
        A, W, _ = _gauss_operands(M, N, K, dt)
        out = _fn(dt)(A, W, Nn.EPI_BF16, alpha=0.866)
        _check_store_gauss(out, A.double() @ W.double().t(), dt, 0.866, f"{name} ({M}, {N}, {K})")


# ---- the 128-column kernel: K loops shorter than, equal to and one longer than its stage ring --------------------------------------
SHORT_K = [
    # N, the M values, the K values, expected choice of every (M, K), epilogues, which variant
    (128, (1, 63, 64, 65, 127, 128, 129), (64, 128, 192, 256, 320), T(64, 4), ("store", "resid"), "64-row tiles, four stages (PER = 6)"),
    (4608, (520,), (64, 128, 192, 256, 320), T(128, 4), ("store", "resid"), "128-row tiles, four stages (PER = 8: the other vmcnt immediates)"),
    (1536, (2816,), (64, 128, 192), T(128, 2), ("store", "resid"), "128-row tiles, two stages"),
]


@pytest.mark.parametrize("N,Ms,Ks,want,epis,why", SHORT_K, ids=["64x4", "128x4", "128x2"])
def test_tile_kernel_short_k_exact(N, Ms, Ks, want, epis, why):
    """nk = 1 .. 5 K-tiles against NST = 4 stages (fewer tiles than stages, as many, one more) and against the double buffer."""
    for M in Ms:
        for K in Ks:
            _assert_choice(M, N, K, want)
            ops = _exact_operands(M, N, K)
            for dt, name in DTYPES:
                _check_exact(_fn(dt), dt, ops, epis, f"{name} ({M}, {N}, {K})")


# ---- split-K with the engine's workspace -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_engine():
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine
    from esmdiff_amd.weights import random_init_state_dict
    eng = Engine(TINY, random_init_state_dict(TINY, seed=1), max_batch=8, max_len=300)
    yield eng
    eng.close()


def _splitk_rule(M, N, K, ws_floats):
    """choose_gemm's split factor restated: for K >= 2048 below the small-batch switch, the largest divisor of K / 64 that is <= 8
    and keeps tiles_n * S <= 96, if S planes of the row-padded product fit the workspace."""
    if M >= SMALL_MAX_ROWS or not ws_floats or K < 2048:
        return 1
    S = next((c for c in range(8, 1, -1) if (K // 64) % c == 0 and (N // 128) * c <= 96), 1)
    return S if S * ((M + 127) // 128) * 128 * N <= ws_floats else 1


def _tile_rule(M, N, S):
    """rows per tile (small_tile_mi below the small-batch switch) and LDS stages (tiles * S <= 256) of the 128-column kernel."""
    rows = 64 if M < SMALL_MAX_ROWS and ((M + 127) // 128) * (N // 128) * S <= 128 else 128
    return rows, 4 if -(-M // rows) * (N // 128) * S <= 256 else 2


SPLITK = [
    # (N, K), the M values, expected S, why
    ((1536, 2048), (1, 129, 774), 8, "four K-tiles per slice: as many as stages"),
    ((1536, 2112), (1, 129, 774), 3, "S = 3, eleven K-tiles per slice"),
    ((1536, 2176), (1, 129, 774), 2, "S = 2, seventeen K-tiles per slice"),
    ((128, 2048), (240,), 8, "one column tile"),
]


@pytest.mark.parametrize("NK,Ms,S,why", SPLITK, ids=[f"{n}x{k}" for (n, k), *_ in SPLITK])
def test_split_k_exact(tiny_engine, NK, Ms, S, why):
    """esmdiff_gemm_bf16_ws: K slices into the engine's workspace + splitk_reduce_kernel.  Integer slices sum exactly in f32."""
    N, K = NK
    ws = tiny_engine.gemm_workspace_floats
    assert ws > 0
    for M in Ms:
        assert _splitk_rule(M, N, K, ws) == S
        rows, stages = _tile_rule(M, N, S)
        _assert_choice(M, N, K, T(rows, stages, S), ws)
        assert _choice(M, N, K, 0)["S"] == 1              # ... and without a workspace nothing is split
        ops = _exact_operands(M, N, K)
        _check_exact(_fn(BF16, tiny_engine), BF16, ops, ("store", "resid", "bias"), f"split-K S = {S} ({M}, {N}, {K})")
        del ops
        _check_inexact(_fn(BF16, tiny_engine), BF16, M, N, K, ("gelu",), f"split-K S = {S} ({M}, {N}, {K})", splitk=True)


# ---- the raw K-slice planes the add+LayerNorm kernel sums -----------------------------------------------------------------------
def _partial_splits_rule(N, K):
    """gemm_partial_splits restated: the largest divisor of K / 64 that is <= 8, leaves every slice >= 6 K-tiles and keeps
    tiles_n * S <= 96; else one raw plane."""
    nk = K // 64
    return next((c for c in range(8, 1, -1) if nk % c == 0 and nk // c >= 6 and (N // 128) * c <= 96), 1)


PLANES = [((1536, 384), 1), ((1536, 768), 2), ((1536, 2048), 4), ((2048, 4096), 4)]


@pytest.mark.parametrize("NK,S", PLANES, ids=[f"{n}x{k}" for (n, k), _ in PLANES])
def test_k_slice_planes_exact(tiny_engine, NK, S):
    """esmdiff_branch_linear_layernorm: x += 0.5 * (A W^T) from S raw planes, exact; y = LayerNorm(x) w + b against float64 by the
    bar of test_branch_linear_layernorm_small_batch.  S is a function of (N, K) only: every M expects the same."""
    N, K = NK
    assert _partial_splits_rule(N, K) == S
    for M in (3, 129, 1151):
        A32, W32, x0, _, ref = _exact_operands(M, N, K)
        g = torch.Generator(device="cuda").manual_seed(N + K + M)
        w, b = torch.randn(N, generator=g, device="cuda"), torch.randn(N, generator=g, device="cuda")
        want_x = (x0.double() + ref * 0.5).float()
        for bias in (b, None):
            first = None
            for _ in range(2):
                x = x0.clone()
                y, got_s = tiny_engine.branch_linear_layernorm(A32.to(BF16), W32.to(BF16), x, 0.5, w, bias)
                assert got_s == S, f"({M}, {N}, {K}): {got_s} planes, the documented rule gives {S}"
                _same(x, want_x, f"planes S = {S} ({M}, {N}, {K}) x")
                if first is None:
                    first = y
            assert torch.equal(_bits(y), _bits(first))
            want_y = torch.nn.functional.layer_norm(want_x.double(), (N,), w.double(), None if bias is None else bias.double(), 1e-5)
            err = (y.double() - want_y).abs()
            assert float((err - want_y.abs() * 2 ** -8).max()) < 2e-3, float(err.max())


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,ldc_pad,why", [(200, 192, 128, 0, "N % 128 != 0"), (200, 256, 96, 0, "K % 64 != 0"),
                                               (200, 256, 128, 2, "ldc % 4 != 0")])
def test_refused_shapes_launch_nothing(tiny_engine, M, N, K, ldc_pad, why):
    """Refused before any launch: an error, and the sentinel-filled output is untouched."""
    from esmdiff_amd import _native as Nn
    for dt, fn in ((BF16, _fn(BF16)), (F16, _fn(F16)), (BF16, tiny_engine.gemm)):
        A = torch.ones(M, K, dtype=dt, device="cuda")
        W = torch.ones(N, K, dtype=dt, device="cuda")
        bias = torch.zeros(N, device="cuda")
        for epi, odt in ((Nn.EPI_BIAS_F32, torch.float32), (Nn.EPI_BF16, dt)):
            o = torch.full((M, N + ldc_pad), 3.0, dtype=odt, device="cuda")
            with pytest.raises(RuntimeError, match="libesmdiff_hip error"):
                fn(A, W, epi, out=o, bias=bias)
            torch.cuda.synchronize()
            assert bool((o == 3.0).all()), why


def test_describe_gemm_choice_refuses_what_the_launcher_refuses():
    import ctypes
    from esmdiff_amd import _native as Nn
    v = [ctypes.c_int32(-1) for _ in range(4)]
    for M, N, K in ((0, 128, 64), (5, 192, 64), (5, 128, 96)):
        assert Nn.lib().esmdiff_describe_gemm_choice(M, N, K, 0, *[ctypes.byref(x) for x in v]) != 0
    assert [x.value for x in v] == [-1] * 4
