"""The ABI's caller's-stream contract, held on a non-default stream (include/esmdiff_hip.h: "All work is enqueued on the caller's
hipStream_t; no entry synchronises the stream except where stated").

Every case runs through tests/stream_order.py: once on the null stream, once on a torch.cuda.Stream that begins with a device-side
delay, with inputs that arrive late on that stream and a clone() of every output behind the call.  Outputs must be the null-stream
run's bit for bit (every kernel here is deterministic; the analysis entries accumulate with integer atomics only), an asynchronous
entry must come back while the stream is still busy, and an entry documented to synchronise the stream must come back with it idle.

One side stream for the whole module; no queue-related environment variable; no graph capture.  Engines: four TINY ones (bf16 with
the geometric weights, f16, f32, f32_split), one production-width two-block engine for the device-side samplers, and the TINY
structure decoder and encoder as their own tests build them, each alive for one test only."""
import ctypes
import functools
import time

import pytest
import torch

from tests.stream_order import Clock, bits_equal, run_both

pytestmark = pytest.mark.gpu

MASK, V = 4096, 4101
SENTINEL = -7.0
BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _tokens(B, L, g, masked=0.5):
    """(seq, x, x0): per-sample sequences with BOS / EOS, structure tokens with a share of MASK, and the same without MASK."""
    seq = torch.randint(4, 24, (B, L), generator=g)
    seq[:, 0], seq[:, -1] = 0, 2
    x0 = torch.randint(0, 4096, (B, L), generator=g)
    x = x0.clone()
    x[torch.rand(B, L, generator=g) < masked] = MASK
    x[:, 0], x[:, -1] = 4098, 4097
    return seq, x, x0


def _tf(sigmas, dim=256):
    from esmdiff_amd.schedule import timestep_embedding
    return timestep_embedding(torch.tensor(sigmas, dtype=F32), dim)


def _cuda(ts):
    return [t.cuda() for t in ts]


def _pair(mk):
    """fresh / stale of a case from mk(kind) (0: fresh, 1: stale), each built once."""
    return functools.lru_cache(None)(lambda: _cuda(mk(0))), functools.lru_cache(None)(lambda: _cuda(mk(1)))


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clock():
    """The module's one side stream and its calibrated delay.  On the way out: the figures EXPERIMENTS.md records."""
    c = Clock()
    yield c
    worst = c.worst()
    if worst is not None:
        print(f"MEASURED stream order: {len(c.reports)} cases, {c.cycles_per_ms:.0f} spin cycles per ms; largest host return "
              f"{worst.host_ms:.2f} ms ({worst.name}) -> delay {worst.delay_ms:.0f} ms; smallest delay "
              f"{min(r.delay_ms for r in c.reports):.0f} ms")


@pytest.fixture(scope="module")
def tiny():
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine
    from esmdiff_amd.weights import random_init_state_dict
    e = Engine(TINY, random_init_state_dict(TINY, seed=1, with_geom=True), max_batch=8, max_len=290)
    yield e
    e.close()


@pytest.fixture(scope="module")
def alt():
    """precision -> a TINY engine of the other three precisions, built when first asked for."""
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine
    from esmdiff_amd.weights import random_init_state_dict
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = Engine(TINY, random_init_state_dict(TINY, seed=1), max_batch=2, max_len=60, precision=precision)
        return made[precision]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def wide():
    from esmdiff_amd.config import ModelConfig
    from esmdiff_amd.engine import Engine
    from esmdiff_amd.weights import random_init_state_dict
    cfg = ModelConfig(n_layers=2)
    e = Engine(cfg, random_init_state_dict(cfg, seed=11), max_batch=9, max_len=258)
    yield e
    e.close()


def _check(rep, busy):
    print(f"MEASURED stream order {rep.name}: host return {rep.host_ms:.3f} ms, delay {rep.delay_ms:.0f} ms, "
          f"busy_on_return {rep.busy_on_return}, mismatches {rep.mismatches}")
    assert rep.ok, (rep.name, rep.mismatches)
    if busy is not None:
        assert rep.busy_on_return == busy, (rep.name, "busy_on_return", rep.busy_on_return, "host ms", rep.host_ms)


# ---- a. the harness sees a disorder ---------------------------------------------------------------------------------------------
def test_a_launch_on_the_null_stream_is_reported(clock):
    """esmdiff_layernorm_bf16 called with stream 0 while its input is produced late on S: the null stream is not ordered against
    a non-blocking stream, so the kernel normalises the stale rows and the harness must say so."""
    from esmdiff_amd import _native as N
    from esmdiff_amd.engine import layernorm_bf16
    M, D = 8, 512
    w = (1 + 0.1 * torch.randn(D, generator=_gen(1))).cuda()
    fresh, stale = _pair(lambda k: [torch.randn(M, D, generator=_gen(10 + k)) * 3 + k])

    def on_stream_0(b):
        y = b[1]
        N.check(N.lib().esmdiff_layernorm_bf16(ctypes.c_void_p(b[0].data_ptr()), ctypes.c_void_p(w.data_ptr()), None,
                                               ctypes.c_void_p(y.data_ptr()), M, D, ctypes.c_void_p(0)))
        return y
    rep = run_both(clock, "planted: layernorm on stream 0", fresh, stale, on_stream_0,
                   outputs=lambda: [torch.full((M, D), SENTINEL, dtype=BF16, device="cuda")])
    print(f"MEASURED stream order {rep.name}: mismatches {rep.mismatches}")
    assert not rep.ok and rep.busy_on_return
    of_stale = layernorm_bf16(stale()[0], w, None)
    torch.cuda.synchronize()
    assert bits_equal(rep.got[0], of_stale)
    assert bits_equal(rep.ref[0], layernorm_bf16(fresh()[0], w, None))
    # the same call on the caller's stream is in order
    _check(run_both(clock, "layernorm on S", fresh, stale, lambda b: layernorm_bf16(b[0], w, None)), True)


def test_a_interior_launch_on_the_null_stream_is_reported(clock):
    """A two-kernel entry that keeps its intermediate in a workspace of its own, as the engine does: LayerNorm into the workspace on
    S, then esmdiff_layernorm_16in of the workspace into the output — planted on stream 0.  The second kernel never reads the late
    input, and its output is written once: it can be caught only because the workspace holds the intermediate of OTHER inputs when it
    runs early (the harness's null-stream call on the stale data, made after the reference run).  Its output must be the two
    LayerNorms of the stale rows; with both kernels on S the case is in order."""
    from esmdiff_amd import _native as N
    from esmdiff_amd.engine import layernorm_16in, layernorm_bf16
    M, D = 8, 512
    w = (1 + 0.1 * torch.randn(D, generator=_gen(2))).cuda()
    work = torch.zeros(M, D, dtype=BF16, device="cuda")             # the "engine-owned" intermediate, alive across calls
    fresh, stale = _pair(lambda k: [torch.randn(M, D, generator=_gen(20 + k)) * 3 + k])
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def two_kernels(second_stream):
        def call(b):
            x, y = b
            N.check(N.lib().esmdiff_layernorm_bf16(p(x), p(w), None, p(work), M, D,
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            N.check(N.lib().esmdiff_layernorm_16in(0, p(work), p(w), None, p(y), M, D, second_stream()))
            return y
        return call
    outputs = lambda: [torch.full((M, D), SENTINEL, dtype=BF16, device="cuda")]
    rep = run_both(clock, "planted: interior kernel on stream 0", fresh, stale, two_kernels(lambda: ctypes.c_void_p(0)),
                   outputs=outputs)
    print(f"MEASURED stream order {rep.name}: mismatches {rep.mismatches}")
    assert not rep.ok and rep.busy_on_return
    of_stale = layernorm_16in(layernorm_bf16(stale()[0], w, None), w, None)
    torch.cuda.synchronize()
    assert bits_equal(rep.got[0], of_stale)
    assert bits_equal(rep.ref[0], layernorm_16in(layernorm_bf16(fresh()[0], w, None), w, None))
    on_s = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _check(run_both(clock, "two kernels on S", fresh, stale, two_kernels(on_s), outputs=outputs), True)


# ---- b. asynchronous entries ----------------------------------------------------------------------------------------------------
ENGINE_ENTRIES = ["forward_logits", "forward_logits_sigmas", "embeddings", "ddpm_step", "ddpm_step_margin", "ddpm_step_rows",
                  "gibbs_step", "gibbs_step_rows", "logit_error_stats", "q_xt", "nelbo_rows", "nelbo_eval", "set_frames_forward",
                  "forward_logits_needed"]


def _engine_case(name, eng, B, L):
    """(fresh, stale, call) of one engine entry at (B, L)."""
    from esmdiff_amd.engine import Engine
    ld = eng.ld_logits

    def base(k):
        g = _gen(1000 * (k + 1) + B * L + len(name))
        return (g,) + _tokens(B, L, g)

    def logits(g):
        return torch.randn(B, L, ld, generator=g) * 3

    def out():
        return torch.full((B, L, ld), SENTINEL)

    def per_sample(g):
        return torch.rand(B, generator=g) * 0.8 + 0.1

    if name in ("forward_logits", "forward_logits_sigmas", "embeddings", "forward_logits_needed"):
        def mk(k):
            g, seq, x, _ = base(k)
            tf = _tf([0.2 + 0.05 * b + 0.4 * k for b in range(B)]) if name == "forward_logits_sigmas" else _tf([0.3 + 0.4 * k])[0]
            return [x, seq, tf, out()]
        if name == "embeddings":
            def call(b):
                eng.forward_logits(b[0], b[1], b[2], out=b[3], check_ids=False)
                return eng.embeddings(B, L)
        elif name == "forward_logits_needed":
            call = lambda b: eng.forward_logits_needed(b[0], b[1], b[2], b[3])
        else:
            call = lambda b: eng.forward_logits(b[0], b[1], b[2], out=b[3], check_ids=False)
    elif name == "ddpm_step":
        def mk(k):
            g, seq, x, _ = base(k)
            return [x, logits(g)]
        call = lambda b: eng.ddpm_step(b[0], b[1], 0.5, 0.46, seed=5, sample_offset=3, step=1)
    elif name == "ddpm_step_margin":
        def mk(k):
            g, seq, x, _ = base(k)
            return [x, logits(g), torch.full((B,), k, dtype=torch.int32)]
        call = lambda b: [eng.ddpm_step_margin(b[0], b[1], 0.5, 0.46, final=False, seed=5, sample_offset=3, step=1, margin=1.5,
                                               flags=b[2]), b[2]]
    elif name == "ddpm_step_rows":
        def mk(k):
            g, seq, x, _ = base(k)
            params = torch.from_numpy(Engine.sample_step_params_host([3 + b + 10 * k for b in range(B)], 0.5 + 0.2 * k,
                                                                     0.46 - 0.2 * k, 1 + k, 0))
            return [x, logits(g), params, torch.full((B,), k, dtype=torch.int32), torch.full((B,), 0.0 if k else float("inf"))]
        call = lambda b: [eng.ddpm_step_rows(b[0], b[1], b[2], seed=5, eps=0.01, flags=b[3], gaps=b[4]), b[3], b[4]]
    elif name == "gibbs_step":
        def mk(k):
            g, seq, x, _ = base(k)
            return [x, seq, logits(g), torch.full((B,), 3 - 2 * k, dtype=torch.int32)]
        call = lambda b: eng.gibbs_step(b[0], b[1], b[2], 1.0, 0.9, b[3], seed=5, sample_offset=0, step=1)
    elif name == "gibbs_step_rows":
        def mk(k):
            g, seq, x, _ = base(k)
            params = torch.from_numpy(Engine.gibbs_step_params_host([b + 10 * k for b in range(B)], 1 + k, [3 - 2 * k] * B))
            return [x, seq, logits(g), params, torch.full((B,), k, dtype=torch.int32),
                    torch.full((B, 2), 0.0 if k else float("inf"))]
        call = lambda b: [eng.gibbs_step_rows(b[0], b[1], b[2], 1.0, 0.9, b[3], seed=5, pair_bound=0.01, entropy_bound=0.01,
                                              flags=b[4], gaps=b[5]), b[4], b[5]]
    elif name == "logit_error_stats":
        def mk(k):
            g, seq, x, _ = base(k)
            a = logits(g)
            return [a, a + 0.01 * torch.randn(B, L, ld, generator=g), x]
        call = lambda b: eng.logit_error_stats(b[0], b[1], b[2])
    elif name == "q_xt":
        def mk(k):
            g, seq, x, x0 = base(k)
            return [x0, seq, per_sample(g), torch.rand(B, L, generator=g)]
        call = lambda b: eng.q_xt(b[0], b[2], sequence_tokens=b[1], coupled=True, u=b[3])
    elif name == "nelbo_rows":
        def mk(k):
            g, seq, x, x0 = base(k)
            return [logits(g), x, x0, per_sample(g)]
        call = lambda b: eng.nelbo_rows(b[0], b[1], b[2], b[3], check_ids=False)
    elif name == "nelbo_eval":
        def mk(k):
            g, seq, x, x0 = base(k)
            return [seq, x0, _tf([0.2 + 0.05 * b + 0.4 * k for b in range(B)]), per_sample(g), per_sample(g),
                    torch.rand(B, L, generator=g)]
        call = lambda b: eng.nelbo_eval(b[0], b[1], b[2], b[3], b[4], u=b[5], return_log_p=True, check_ids=False)
    elif name == "set_frames_forward":
        def mk(k):
            g, seq, x, _ = base(k)
            return _frames(B, L, g) + [x, seq, out()]

        def call(b):
            eng.set_frames(b[0], b[1], b[2])
            lg = eng.forward_logits(b[3], b[4], None, out=b[5], check_ids=False)
            eng.set_frames(None)
            return lg
    else:
        raise KeyError(name)
    return _pair(mk) + (call,)


def _frames(B, L, g):
    """[rot, trans, has_frame u8] of a random finite backbone."""
    from esmdiff_amd.geometry import build_affine3d_from_coordinates
    ca = torch.cumsum(torch.randn(B, L, 3, generator=g) * 2.2, 1)
    xyz = torch.stack([ca + torch.randn(B, L, 3, generator=g) * 0.8, ca, ca + torch.randn(B, L, 3, generator=g) * 0.8], 2)
    rot, trans, has = build_affine3d_from_coordinates(xyz)
    return [rot, trans, has.to(torch.uint8)]


@pytest.mark.parametrize("name", ENGINE_ENTRIES)
@pytest.mark.parametrize("B,L", [(2, 60), (8, 290)])
def test_b_engine_entry_is_asynchronous_and_in_order(clock, tiny, B, L, name):
    """(2, 60): the small-batch path on one queue.  (8, 290): 2 320 tokens, the regular path with the second half of the batch on the
    engine's side stream, forked from and joined back into the caller's stream."""
    plan = tiny.describe_plan(B, L)
    assert ("small-batch" in plan) == (B * L < 1152)
    if (B, L) == (8, 290):
        assert "streams=2" in plan, plan
    _check(run_both(clock, f"{name} bf16 ({B}, {L})", *_engine_case(name, tiny, B, L)), True)


@pytest.mark.parametrize("precision", ["f16", "f32", "f32_split"])
def test_b_forward_of_the_other_precisions(clock, alt, precision):
    """Their linears and attention go through other launchers (gemm_split.hip, attention_split.hip, strict.hip)."""
    _check(run_both(clock, f"forward_logits {precision} (2, 60)", *_engine_case("forward_logits", alt(precision), 2, 60)), True)


def _randn(*shape, seed, scale=1.0, dtype=F32):
    return (torch.randn(*shape, generator=_gen(seed)) * scale).to(dtype)


def _kernel_case(name, tiny, alt):
    """(fresh, stale, call) of one kernel-level entry, small, as its own test calls it."""
    from esmdiff_amd import _native as N
    from esmdiff_amd import engine as E
    D, H = 512, 8
    if name in ("gemm_bf16", "gemm_f16", "gemm_f32"):
        dt = {"gemm_bf16": BF16, "gemm_f16": F16, "gemm_f32": F32}[name]
        mk = lambda k: [_randn(200, 192, seed=1 + k, dtype=dt), _randn(256, 192, seed=3 + k, scale=192 ** -0.5, dtype=dt)]
        if name == "gemm_f32":
            call = lambda b: E.gemm_f32(b[0], b[1])
        else:
            fn = E.gemm_bf16 if name == "gemm_bf16" else E.gemm_f16
            call = lambda b: fn(b[0], b[1], N.EPI_BF16)
    elif name in ("split_rows+gemm_split", "gemm_split_k"):
        M, Nn, K = (130, 256, 128) if name == "split_rows+gemm_split" else (5, 256, 768)
        w3, inv = E.split_weight(_randn(Nn, K, seed=5, scale=K ** -0.5).cuda())
        torch.cuda.synchronize()
        mk = lambda k: [_randn(M, K, seed=7 + k, scale=1.0 + k), _randn(M, Nn, seed=9 + k)]
        if name == "gemm_split_k":
            def call(b):
                a3, rs = E.split_rows(b[0])
                parts = E.gemm_split_k(a3, rs, w3, inv, b[1], 3, div=1.1547005)
                return [b[1], parts[:, :M]]
        else:
            def call(b):
                a3, rs = E.split_rows(b[0])
                return [a3, rs, E.gemm_split(a3, rs, w3, inv, Nn)]
    elif name == "branch_linear_layernorm":
        K = Nn = 1536
        mk = lambda k: [_randn(3, K, seed=1 + k, dtype=BF16), _randn(Nn, K, seed=3 + k, scale=K ** -0.5, dtype=BF16),
                        _randn(3, Nn, seed=5 + k, scale=3.0), 1 + 0.1 * _randn(Nn, seed=7 + k), _randn(Nn, seed=9 + k)]
        call = lambda b: [tiny.branch_linear_layernorm(b[0], b[1], b[2], 0.866, b[3], b[4])[0], b[2]]
    elif name in ("layernorm_bf16", "layernorm_16in", "add_layernorm", "layernorm_f32rows"):
        def mk(k):
            x = _randn(8, D, seed=1 + k, scale=3.0) + 0.5 * k
            rows = {"layernorm_16in": [x.to(BF16)], "add_layernorm": [x, _randn(8, D, seed=3 + k, dtype=BF16),
                                                                     _randn(8, D, seed=5 + k, dtype=BF16)]}.get(name, [x])
            return rows + [1 + 0.1 * _randn(D, seed=7 + k), _randn(D, seed=9 + k)]
        if name == "layernorm_bf16":
            call = lambda b: E.layernorm_bf16(b[0], b[1], b[2])
        elif name == "layernorm_16in":
            call = lambda b: E.layernorm_16in(b[0], b[1], b[2])
        elif name == "add_layernorm":
            call = lambda b: [E.add_layernorm(BF16, b[0], b[1], b[2], True, b[3], b[4]), b[0]]
        else:
            call = lambda b: [E.layernorm_f32rows(b[0], b[1], b[2], split=False)] + \
                list(E.layernorm_f32rows(b[0], b[1], b[2], split=True))
    elif name == "swiglu_f32":
        mk = lambda k: [_randn(8, 512, seed=1 + k, scale=2.0)]
        call = lambda b: E.swiglu_f32(b[0])
    elif name in ("qk_norm_rope", "qk_norm_rope_f32", "attention_L65", "v_split", "attention_f32_parts"):
        B, L = (1, 65) if name == "attention_L65" else (2, 33)
        dt = BF16 if name in ("qk_norm_rope", "attention_L65") else F32
        mk = lambda k: [_randn(B * L, 3 * D, seed=1 + k, dtype=dt), 1 + 0.1 * _randn(D, seed=3 + k), 1 + 0.1 * _randn(D, seed=5 + k)]
        if name == "qk_norm_rope":
            call = lambda b: tiny.qk_norm_rope(b[0], b[1], b[2], B, L, H)
        elif name == "qk_norm_rope_f32":
            f32 = alt("f32")
            call = lambda b: f32.qk_norm_rope_f32(b[0], b[1], b[2], B, L, H)
        elif name == "attention_L65":
            call = lambda b: tiny.attention(b[0], b[1], b[2], B, L)
        elif name == "v_split":
            call = lambda b: E.v_split(b[0], 1.0)
        else:
            mk = lambda k: [_randn(B * L, D, seed=1 + k), _randn(B * L, D, seed=3 + k), _randn(B * L, 3 * D, seed=5 + k)]
            call = lambda b: E.attention_f32_parts(b[0], b[1], b[2], B, L, H)
    elif name == "attention_16_parts":
        B, L = 2, 65
        mk = lambda k: [_randn(B * L, D, seed=1 + k, scale=0.18, dtype=BF16), _randn(B * L, D, seed=3 + k, dtype=BF16),
                        _randn(B * L, 3 * D, seed=5 + k, dtype=BF16)]
        call = lambda b: E.attention_16_parts(b[0], b[1], b[2], B, L, H)
    elif name == "embed_rows":
        def mk(k):
            g = _gen(20 + k)
            seq, x, _ = _tokens(2, 9, g)
            return [seq, x, _randn(64, D, seed=1 + k), _randn(V, D, seed=3 + k), _randn(D, seed=5 + k), _randn(D, seed=7 + k)]
        call = lambda b: E.embed_rows(b[0], b[1], b[2], b[3], b[4], b[5], 0)
    elif name == "gather_table_rows":
        mk = lambda k: [torch.randint(0, V, (20,), generator=_gen(1 + k)), _randn(V, D, seed=3 + k)]
        call = lambda b: E.gather_table_rows(b[0], b[1])
    elif name == "sigma_mlp":
        mk = lambda k: [_tf([0.1 + k, 0.5 + k, 0.9 + k]), _randn(D, 256, seed=1 + k, scale=1 / 16), _randn(D, seed=3 + k),
                        _randn(D, D, seed=5 + k, scale=D ** -0.5), _randn(D, seed=7 + k)]
        call = lambda b: E.sigma_mlp(*b)
    elif name == "convert_weight":
        mk = lambda k: [_randn(1000, seed=1 + k, scale=10.0)]
        call = lambda b: E.convert_weight(b[0], BF16)
    elif name == "interleave_swiglu":
        mk = lambda k: [_randn(128, 64, seed=1 + k)]
        call = lambda b: E.interleave_swiglu(b[0], BF16)
    elif name == "math_eval":
        def mk(k):
            rec = torch.randint(0, 256, (5000, 32), generator=_gen(3 + k), dtype=torch.uint8)
            return [torch.rand(100000, generator=_gen(1 + k)) * (20 + k) + 1e-3, rec]
        call = lambda b: [E.math_eval("sampler", "exp", b[0]), E.math_eval("score", "log", b[0]), E.math_eval("gibbs", "noise", b[0]),
                          E.math_eval("gibbs", "philox", b[1])]
    else:
        raise KeyError(name)
    return _pair(mk) + (call,)


KERNEL_ENTRIES = ["gemm_bf16", "gemm_f16", "gemm_f32", "split_rows+gemm_split", "gemm_split_k", "branch_linear_layernorm",
                  "layernorm_bf16", "layernorm_16in", "add_layernorm", "layernorm_f32rows", "swiglu_f32", "qk_norm_rope",
                  "qk_norm_rope_f32", "v_split", "attention_L65", "attention_f32_parts", "attention_16_parts", "embed_rows",
                  "gather_table_rows", "sigma_mlp", "convert_weight", "interleave_swiglu", "math_eval"]


@pytest.mark.parametrize("name", KERNEL_ENTRIES)
def test_b_kernel_entry_is_asynchronous_and_in_order(clock, tiny, alt, name):
    _check(run_both(clock, name, *_kernel_case(name, tiny, alt)), True)


# ---- c. a chain -----------------------------------------------------------------------------------------------------------------
def test_c_host_loop_chain_behind_one_delay(clock, tiny):
    """ddpm_sample(..., sample_index=...) is a host loop of forward + ddpm_step_rows.  The same loop, T = 3, at (8, 290) with every
    launch on S behind ONE delay (the per-step parameter records are uploaded beforehand: the wrapper's own upload from pageable
    memory waits for the stream): call N + 1 reuses the workspace that call N's side stream wrote.  Ids as on the null stream,
    and as Engine.ddpm_sample gives them."""
    from esmdiff_amd.engine import Engine
    from esmdiff_amd.schedule import ddpm_schedule
    B, L, T, seed = 8, 290, 3, 5
    sch = ddpm_schedule(T, eps=0.3)
    index = [11 + 2 * b for b in range(B)]
    tf = tiny.conditioning_rows(sch.t_freq).float().cuda()
    params = [torch.from_numpy(Engine.sample_step_params_host(index, 0.0 if i == T else float(sch.mc_t[i]),
                                                              0.0 if i == T else float(sch.mc_s[i]), i, int(i == T))).cuda()
              for i in range(T + 1)]

    def mk(k):
        seq, x, _ = _tokens(B, L, _gen(77 + k), masked=0.6)
        return [seq, x, torch.full((B, L, tiny.ld_logits), SENTINEL)]

    def chain(b):
        seq, x, logits = b
        for i in range(T + 1):
            lg = tiny.forward_logits(x, seq, tf[i], out=logits, check_ids=False)
            tiny.ddpm_step_rows(x, lg, params[i], seed=seed)
        return x
    fresh, stale = _pair(mk)
    rep = run_both(clock, "chain: 4 x (forward + ddpm_step_rows) (8, 290)", fresh, stale, chain)
    _check(rep, True)
    seq, x, _ = fresh()
    want = tiny.ddpm_sample(seq, sch, seed=seed, input_prior=x, sample_index=index)
    torch.cuda.synchronize()
    assert torch.equal(rep.got[0], want)
    assert int((want == MASK).sum()) == 0 and not torch.equal(want, x)


# ---- d. entries that are documented to wait -------------------------------------------------------------------------------------
def _every_second(B, L, g):
    seq, _, x0 = _tokens(B, L, g)
    x = x0.clone()
    x[:, 0::2] = MASK
    return seq, x


# name -> (needed rows, step-0 sharing, final skip, the [host] arrays in pinned memory)
DDPM_OPTIONS = {"needed_rows": (True, False, False, False), "all_off": (False, False, False, False),
                "shortcuts": (True, True, True, False), "all_off_pinned": (False, False, False, True)}


@pytest.mark.parametrize("options", list(DDPM_OPTIONS))
def test_d_ddpm_sample_on_the_device(clock, wide, options):
    """esmdiff_ddpm_sample at (9, 258) (the 4 + 5 cut), prior every_second, T = 3.  Its [host] arrays mc_t, mc_s and t_freq are
    overwritten with other valid values as soon as the call has returned: the header says they are consumed by then, in pageable and
    in pinned memory (an upload straight from a pinned array would read it when the stream gets there).  With needed rows, step-0
    sharing and the final skip all off the entry has no wait: it must come back while the stream is still delayed, as
    INTEGRATION.md promises a caller that must not block its thread."""
    from esmdiff_amd.schedule import ddpm_schedule
    B, L, T = 9, 258, 3
    needed, share, skip, pinned = DDPM_OPTIONS[options]
    sch = ddpm_schedule(T, eps=0.3)
    host = [sch.mc_t[:T].float().contiguous(), sch.mc_s[:T].float().contiguous(),
            wide.conditioning_rows(sch.t_freq).float().contiguous()]
    other = [torch.full((T,), 0.7), torch.full((T,), 0.2), _tf([2.0, 1.5, 1.0, 0.5])]
    held = []

    def call(b):
        held.append([t.clone().pin_memory() if pinned else t.clone() for t in host])
        return wide._ddpm_sample_device(b[0], b[1], T, *held[-1], 5, 3)

    def scribble():
        for t, o in zip(held[-1], other):
            t.copy_(o)
    fresh, stale = _pair(lambda k: list(_every_second(B, L, _gen(9258 + k))))
    wide.set_needed_rows(needed)
    wide.set_step0_sharing(share)
    wide.set_final_skip(skip)
    try:
        rep = run_both(clock, f"ddpm_sample device ({options}) (9, 258)", fresh, stale, call, after_return=scribble)
    finally:
        wide.set_needed_rows(True)
        wide.set_step0_sharing(False)
        wide.set_final_skip(False)
    _check(rep, True if not (needed or share or skip) else None)
    assert int((rep.got[0] == MASK).sum()) == 0


def test_d_gibbs_sample_on_the_device(clock, wide):
    """esmdiff_gibbs_sample, T = 3, without and with step-0 sharing; n_unmask_table [host], pageable or pinned, is overwritten after
    the return.  Without the sharing's read-back the entry has no wait."""
    B, L, T = 9, 258, 3
    tab = torch.full((T, B), 20, dtype=torch.int32)
    held = []

    def call(b):
        held.append(tab.clone().pin_memory() if pinned else tab.clone())
        return wide._gibbs_sample_device(b[0], b[1], held[-1], 1.0, 0.9, 5, 3)
    fresh, stale = _pair(lambda k: list(_every_second(B, L, _gen(1258 + k))))
    for share, pinned in ((False, False), (True, False), (False, True)):
        wide.set_step0_sharing(share)
        try:
            rep = run_both(clock, f"gibbs_sample device (sharing {share}, pinned {pinned}) (9, 258)", fresh, stale, call,
                           after_return=lambda: held[-1].fill_(1))
        finally:
            wide.set_step0_sharing(False)
        _check(rep, None if share else True)
        assert int((rep.got[0] != fresh()[1]).sum()) == T * 20 * B


def test_d_ddpm_sample_with_the_longest_schedule(clock, tiny):
    """The [host] arrays at their largest: T = 1025, t_freq of 1 026 x 256 floats (1 MB), on the TINY engine at (2, 60), needed
    rows (inert on the small-batch path), step-0 sharing and the final skip off.  The arrays are overwritten on return; the ids are
    the null-stream run's, and the entry comes back with the stream busy at this size too."""
    from esmdiff_amd.schedule import ddpm_schedule
    B, L, T = 2, 60, 1025
    sch = ddpm_schedule(T)
    host = [sch.mc_t[:T].float().contiguous(), sch.mc_s[:T].float().contiguous(),
            tiny.conditioning_rows(sch.t_freq).float().contiguous()]
    assert host[2].numel() * 4 > 1 << 20
    held = []

    def call(b):
        held.append([t.clone() for t in host])
        return tiny._ddpm_sample_device(b[1], b[0], T, *held[-1], 5, 3)

    def scribble():
        held[-1][0].fill_(0.7), held[-1][1].fill_(0.2), held[-1][2].copy_(held[-1][2].flip(0))

    def mk(k):
        seq, x, _ = _tokens(B, L, _gen(1025 + k), masked=0.9)
        return [x, seq]
    tiny.set_needed_rows(False)
    try:
        rep = run_both(clock, "ddpm_sample device T = 1025 (2, 60)", *_pair(mk), call, after_return=scribble, warm=False)
    finally:
        tiny.set_needed_rows(True)
    _check(rep, True)
    assert int((rep.got[0] == MASK).sum()) == 0


def _chain(n, L, g, atoms=None):
    ca = torch.cumsum(torch.randn(n, L, 3, generator=g, dtype=F64) * 2.2, 1)
    if atoms is None:
        return ca
    return torch.stack([ca + torch.randn(n, L, 3, generator=g, dtype=F64) * (0.6 if a != 1 else 0.0) for a in range(atoms)], 2)


def _sync_case(name, tiny):
    """(fresh, stale, call) of one entry that synchronises `stream`; n = 6 structures of L = 40."""
    from esmdiff_amd import metrics, pairs
    n, L = 6, 40
    two = lambda k: [_chain(n, L, _gen(1 + k)), _chain(n, L, _gen(3 + k))]
    one = lambda k: [_chain(n, L, _gen(1 + k))]
    bb = lambda k: [_chain(n, L, _gen(1 + k), atoms=4)]
    cases = {
        "superpose": (two, lambda b: pairs.superpose(b[0], b[1], None, None, False, ("rmsd", "R", "t"))),
        "tm": (two, lambda b: pairs.tm(b[0], b[1], None, None)),
        "lddt_counts": (two, lambda b: pairs.lddt_counts(b[0], b[1], None, None)),
        "dssp": (bb, lambda b: pairs.dssp(b[0], None, None)),
        "contact_map": (one, lambda b: pairs.contact_map(b[0], None, 8.0, 3)),
        "native_contacts": (two, lambda b: pairs.native_contacts(b[0], b[1], None, None, 8.0, 3, 1.8, 5.0)),
        "backbone_torsions": (bb, lambda b: pairs.backbone_torsions(b[0], None, 4.5)),
        "ramachandran": (bb, lambda b: pairs.ramachandran(b[0], None, 4.5, 36)),
        "pair_msf": (one, lambda b: pairs.pair_msf(b[0], None)),
        "fit": (lambda k: [_chain(n, L, _gen(1 + k)), _chain(1, L, _gen(3 + k))[0]], lambda b: pairs.fit(b[0], None, b[1], None)),
        "moments": (one, lambda b: pairs.moments(b[0], None)),
    }
    if name in cases:
        mk, call = cases[name]
    elif name == "threshold+gromos":
        def mk(k):
            d = torch.rand(n, n, generator=_gen(1 + k), dtype=F64) * 10
            return [(d + d.T) / 2, torch.zeros(n, 1, dtype=torch.int64)]

        def call(b):
            pairs.threshold(b[0], 0, 5.0, False, b[1])
            out, k = pairs.gromos(b[1])
            return [b[1], out[0], k]
    elif name in ("js_pwd", "js_rg", "validity", "bonding_validity"):
        mk = two
        fn = getattr(metrics, name)
        call = lambda b: torch.tensor(list(fn({"target": b[0], "model": b[1]}, rounded=False).values()), dtype=F64)
    elif name == "attention_ragged":
        D = tiny.cfg.d_model
        mk = lambda k: [_randn(2 * 33, 3 * D, seed=1 + k, dtype=BF16), 1 + 0.1 * _randn(D, seed=3 + k), 1 + 0.1 * _randn(D, seed=5 + k)]
        call = lambda b: tiny.attention_ragged(b[0], b[1], b[2], 2, 33, lengths=[33, 17])
    elif name == "attention_16_parts_ragged":
        from esmdiff_amd import engine as E
        D = 512
        mk = lambda k: [_randn(2 * 33, D, seed=1 + k, scale=0.18, dtype=BF16), _randn(2 * 33, D, seed=3 + k, dtype=BF16),
                        _randn(2 * 33, 3 * D, seed=5 + k, dtype=BF16)]
        call = lambda b: E.attention_16_parts(b[0], b[1], b[2], 2, 33, 8, lengths=[33, 17])
    else:
        raise KeyError(name)
    return _pair(mk) + (call,)


SYNC_ENTRIES = ["attention_ragged", "attention_16_parts_ragged", "superpose", "tm", "lddt_counts", "dssp", "contact_map", "native_contacts",
                "backbone_torsions", "ramachandran", "threshold+gromos", "pair_msf", "fit", "moments", "js_pwd", "js_rg", "validity", "bonding_validity"]


@pytest.mark.parametrize("name", SYNC_ENTRIES)
def test_d_entry_that_synchronises_the_stream(clock, tiny, name):
    _check(run_both(clock, name, *_sync_case(name, tiny)), False)


def _decode(dec, tok):
    """StructureDecoder.decode without its range check of the tokens (a read-back that waits for the stream)."""
    from esmdiff_amd import _native as N
    B, L = tok.shape
    out = torch.full((B, L, 3, 3), SENTINEL, device="cuda")
    pl, ptm = torch.full((B, L), SENTINEL, device="cuda"), torch.full((B,), SENTINEL, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    N.check(dec._lib.esmdiff_decoder_decode(dec._h, p(tok), p(out), p(pl), p(ptm), None, B, L, float(dec.cfg.trans_scale),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), dec._h)
    return out, pl, ptm


def test_d_decoder_and_encoder(clock):
    """esmdiff_encoder_encode is documented to synchronise the stream.  esmdiff_decoder_decode is not: the header gives it one wait,
    when a call with ptm / pae finds the pairwise head's workspace too small and grows it.  That wait is held first, on a fresh
    decoder: the call comes back only after the delay in front of it has run.  After that the entry is asynchronous like a forward,
    and is held to that.  StructureDecoder.decode of the Python host, which reads the tokens' range back before the call, gives
    the null-stream answer on the delayed stream too."""
    from esmdiff_amd.config import TINY_DECODER, TINY_ENCODER
    from esmdiff_amd.engine import StructureDecoder, StructureEncoder
    from esmdiff_amd.weights import random_init_decoder_state_dict, random_init_encoder_state_dict
    B, L = 2, 40

    def toks(k):
        tok = torch.randint(0, 4096, (B, L), generator=_gen(40 + k))
        tok[:, 0], tok[:, -1] = 4098, 4097
        return [tok]
    dec = StructureDecoder(TINY_DECODER, random_init_decoder_state_dict(TINY_DECODER, seed=2), max_batch=B, max_len=L)
    try:
        tok = toks(0)[0].cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(clock.stream):
            clock.sleep(50.0)
            t0 = time.perf_counter()
            _decode(dec, tok)
            waited_ms = (time.perf_counter() - t0) * 1e3
        clock.stream.synchronize()
        print(f"MEASURED stream order first decode with ptm behind a 50 ms delay: returned after {waited_ms:.1f} ms")
        assert waited_ms >= 25.0, waited_ms               # it waited for the stream (a launch sequence returns in well under 1 ms)
        _check(run_both(clock, "esmdiff_decoder_decode", *_pair(toks), lambda b: _decode(dec, b[0])), True)
        _check(run_both(clock, "StructureDecoder.decode", *_pair(toks),
                        lambda b: dec.decode(b[0], return_plddt=True, return_ptm=True, return_pae=True)), None)
    finally:
        dec.close()
    # the encoder takes its coordinates from the host: nothing arrives late, the consumer behind the call is what is checked
    xyz = _chain(B, L, _gen(5), atoms=3).float()
    enc = StructureEncoder(TINY_ENCODER, random_init_encoder_state_dict(TINY_ENCODER, seed=1))
    try:
        _check(run_both(clock, "encoder.encode", lambda: [], lambda: [], lambda b: enc.encode(xyz)), False)
    finally:
        enc.close()


# ---- e. state setters against work in flight ------------------------------------------------------------------------------------
def test_e_set_gibbs_options_against_a_step_in_flight(clock, tiny):
    """A gibbs step under invalid_ids = A is queued on S behind the delay; set_gibbs_options(invalid_ids = B) follows before anything
    is synchronised, then a second step from the same tokens.  B forbids exactly what the first step picks, so the two answers
    differ, and a first step that read B's mask gives the second answer."""
    B_, L = 2, 60
    A = list(range(64))

    def mk(k):
        g = _gen(500 + k)
        seq, x, _ = _tokens(B_, L, g, masked=0.7)
        return [x, x.clone(), seq, torch.randn(B_, L, tiny.ld_logits, generator=g) * 3, torch.full((B_,), 4 - 2 * k, dtype=torch.int32)]
    fresh, stale = _pair(mk)
    step = lambda x, b: tiny.gibbs_step(x, b[2], b[3], 1.0, 0.9, b[4], seed=5, sample_offset=0, step=1)
    try:
        tiny.set_gibbs_options(invalid_ids=A)
        b0 = [t.clone() for t in fresh()]
        first = step(b0[0], b0).cpu()
        picked = first[first != fresh()[0].cpu()]
        assert picked.numel() == 4 * B_ and not set(picked.tolist()) & set(A)
        forbid = sorted(set(picked.tolist()))

        def call(b):
            tiny.set_gibbs_options(invalid_ids=A)
            step(b[0], b)
            tiny.set_gibbs_options(invalid_ids=forbid)
            step(b[1], b)
            return [b[0], b[1]]
        rep = run_both(clock, "gibbs_step | set_gibbs_options | gibbs_step", fresh, stale, call)
    finally:
        tiny.set_gibbs_options()
    _check(rep, None)
    assert torch.equal(rep.ref[0].cpu(), first) and not torch.equal(rep.ref[0], rep.ref[1])
    second = rep.ref[1].cpu()
    assert not set(second[second != fresh()[0].cpu()].tolist()) & set(forbid)


def test_e_set_lengths_against_a_forward_in_flight(clock, tiny):
    """Two ragged forwards at (8, 290) with different lengths, the second set_lengths while the first forward is queued."""
    B, L = 8, 290
    lens = ([290, 100, 3, 257, 64, 290, 129, 200], [33, 290, 258, 3, 290, 65, 128, 17])

    def mk(k):
        res = []
        for j, ln in enumerate(lens):
            seq, x, _ = _tokens(B, L, _gen(600 + 10 * k + j))
            pad = torch.arange(L)[None] >= torch.tensor(ln)[:, None]
            seq[pad], x[pad] = 1, 4099
            res += [x, seq, torch.full((B, L, tiny.ld_logits), SENTINEL)]
        return res + [_tf([0.3 + 0.4 * k])[0]]

    def call(b):
        try:
            tiny.set_lengths(lens[0])
            o1 = tiny.forward_logits(b[0], b[1], b[6], out=b[2], check_ids=False)
            tiny.set_lengths(lens[1])
            o2 = tiny.forward_logits(b[3], b[4], b[6], out=b[5], check_ids=False)
        finally:
            tiny.set_lengths(None)
        return [o1, o2]
    rep = run_both(clock, "forward | set_lengths | forward (8, 290)", *_pair(mk), call)
    _check(rep, True)            # set_lengths(None), the last call, waits for nothing: the second forward is still queued
    assert not bits_equal(rep.ref[0], rep.ref[1])


def test_e_set_frames_against_a_forward_in_flight(clock, tiny):
    """Two forwards at (8, 290) with different frames, the second set_frames while the first forward is queued: set_frames copies
    on the caller's stream, so nothing waits and both forwards read their own frames."""
    B, L = 8, 290

    def mk(k):
        g = _gen(700 + k)
        seq, x, _ = _tokens(B, L, g)
        return _frames(B, L, g) + _frames(B, L, g) + [x, seq, torch.full((B, L, tiny.ld_logits), SENTINEL),
                                                      torch.full((B, L, tiny.ld_logits), SENTINEL)]

    def call(b):
        try:
            tiny.set_frames(b[0], b[1], b[2])
            o1 = tiny.forward_logits(b[6], b[7], None, out=b[8], check_ids=False)
            tiny.set_frames(b[3], b[4], b[5])
            o2 = tiny.forward_logits(b[6], b[7], None, out=b[9], check_ids=False)
        finally:
            tiny.set_frames(None)
        return [o1, o2]
    rep = run_both(clock, "set_frames | forward | set_frames | forward (8, 290)", *_pair(mk), call)
    _check(rep, True)
    assert not bits_equal(rep.ref[0], rep.ref[1])
