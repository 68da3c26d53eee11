"""The four-wave 256x256 GEMM (csrc/gemm256w4.hip) on its v_mfma_f32_16x16x32 main loop: every bf16 / f16 epilogue at the
forward's shapes against a float64 A @ W^T, bitwise determinism across launches, and rows that do not depend on M — the
same rows computed inside batches of different sizes, and inside a batch small enough for the 128-column kernel (the
regular forward paths give bitwise equal logits whichever GEMM kernel a batch size selects)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (M, N, K, epilogue): QKV, out-projection, FFN-up, FFN-down, structure-head MLP, the ragged 4101-of-4352 head
SHAPES = [(12900, 4608, 1536, "store"), (12900, 1536, 1536, "resid"), (25800, 8192, 1536, "swiglu"),
          (25800, 1536, 4096, "resid"), (8229, 1536, 4096, "gelu"), (8229, 4352, 1536, "head")]


def _fns(dt):
    from esmdiff_amd.engine import gemm_bf16, gemm_f16
    return gemm_bf16 if dt == torch.bfloat16 else gemm_f16


def _run(dt, epi, A, W, bias=None, x0=None):
    from esmdiff_amd import _native as Nn
    fn = _fns(dt)
    if epi == "store":
        return fn(A, W, Nn.EPI_BF16, alpha=0.866)
    if epi == "swiglu":
        return fn(A, W, Nn.EPI_SWIGLU_BF16)
    if epi == "gelu":
        return fn(A, W, Nn.EPI_BIAS_GELU_BF16, bias=bias)
    if epi == "resid":
        x = x0.clone()
        fn(A, W, Nn.EPI_RESID_F32, out=x, alpha=0.5)
        return x
    o = torch.full((A.shape[0], 4104), -7.0, device="cuda")
    fn(A, W, Nn.EPI_BIAS_F32, out=o, bias=bias, n_valid=4101)
    return o


def _operands(M, N, K, dt, seed, epi):
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(M, K, generator=g, device="cuda").to(dt)
    W = (torch.randn(N, K, generator=g, device="cuda") / K ** 0.5).to(dt)
    if N == 4352:
        W[4101:] = 0
    bias = torch.randn(N, generator=g, device="cuda")
    x0 = torch.randn(M, N, generator=g, device="cuda") if epi == "resid" else None
    return A, W, bias, x0


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("M,N,K,epi", SHAPES)
def test_w4_epilogues_vs_float64(M, N, K, epi, dt):
    """Error against float64 within the bars of tests/test_gpu_kernels.py (which compare against f32 torch)."""
    A, W, bias, x0 = _operands(M, N, K, dt, M + N + K, epi)
    out = _run(dt, epi, A, W, bias, x0)
    ref = A.double() @ W.double().t()
    f16 = dt == torch.float16
    if epi == "store":
        e = (out.double() - ref * 0.866).abs()
        assert float((e - ref.abs() * 0.866 * (2 ** -11 if f16 else 2 ** -8)).max()) < (5e-4 if f16 else 4e-3), float(e.max())
    elif epi == "swiglu":
        r = ref.view(M, N // 64, 2, 32)
        want = (torch.nn.functional.silu(r[:, :, 0]) * r[:, :, 1]).reshape(M, N // 2)
        e = (out.double() - want).abs()
        assert float((e - want.abs() * (2 ** -10 if f16 else 2 ** -7)).max()) < (1.5e-3 if f16 else 1e-2), float(e.max())
    elif epi == "gelu":
        want = torch.nn.functional.gelu(ref + bias.double())
        e = (out.double() - want).abs()
        if f16:
            assert float(e.max()) < 4e-3 and float(e.mean()) < 3e-4, float(e.max())
        else:
            assert float((e - want.abs() * 2 ** -7).max()) < 1e-2 and float(e.mean()) < 2e-3, float(e.max())
    elif epi == "resid":
        assert float((out.double() - (x0.double() + ref * 0.5)).abs().max()) < 1e-3
    else:
        want = (ref + bias.double())[:, :4101]
        assert float((out[:, :4101].double() - want).abs().max()) < (2e-4 if f16 else 1e-3)
        assert torch.equal(out[:, 4101:], bias[4101:4104].expand(M, 3))   # padding columns up to ldc: zero W rows + bias
        assert bool((out[-5:, :4101] != -7.0).all())                 # the ragged last row tile is


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("M,N,K,epi", [(12900, 4608, 1536, "store"), (25800, 8192, 1536, "swiglu"),
                                       (25800, 1536, 4096, "resid"), (8229, 1536, 4096, "gelu"), (8229, 4352, 1536, "head")])
def test_w4_rows_do_not_depend_on_m(M, N, K, epi, dt):
    """Repeated launches give the same bits, and so do the same rows inside a smaller batch (another ragged row tile, other
    tile-to-workgroup assignment) and inside a 200-row batch, which the dispatcher gives to the 128-column kernel."""
    A, W, bias, x0 = _operands(M, N, K, dt, 7 * M + K, epi)
    full = _run(dt, epi, A, W, bias, x0)
    torch.cuda.synchronize()
    assert torch.equal(full, _run(dt, epi, A, W, bias, x0))
    for r0, n in ((1000, 5101), (M - 200, 200)):
        part = _run(dt, epi, A[r0:r0 + n].contiguous(), W, bias, None if x0 is None else x0[r0:r0 + n].contiguous())
        assert torch.equal(part, full[r0:r0 + n]), (r0, n)
