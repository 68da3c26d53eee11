#!/usr/bin/env python3
"""Time the scoring path on an MI355X with HIP events, in one process (EXPERIMENTS.md "Scoring"):

  kernels   esmdiff_nelbo_rows against the existing esmdiff_ddpm_step (Philox, non-final) on the SAME logits, B x L all MASK,
            both through the C ABI with preallocated buffers (no Python allocation or read-back inside the timed window);
            the two are alternated round by round and the medians compared.  CHECK: nelbo_rows <= ddpm_step — it reads the
            same bytes with less arithmetic, and the yardstick is existing code.
  engines   esmdiff_nelbo_eval against a bare esmdiff_forward_logits_sigmas at the same shape on full-size random-init
            engines (bf16, f32_split), all MASK.  CHECK: eval - forward <= ddpm_step + 5 % of the forward (the two small
            kernels and nothing else: no host synchronisation, no copy).  Reports (structure, draw) pairs per second.

    python tools/measure_nelbo.py [--B 100] [--L 258] [--skip-engines] [--json out.json]

Exits 1 when a check fails.  Needs the GPU: there is no CPU path."""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

MASK = 4096


def _timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fa, fb, iters, rounds):
    """Median ms per call of fa and of fb, measured in alternating windows of `iters` calls after a warm-up of both."""
    for _ in range(3):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(_timed(fa, iters))
        tb.append(_timed(fb, iters))
    return ta, tb


def measure_kernels(B=100, L=258, iters=50, rounds=9):
    """nelbo_rows (rows kernel + per-sample reduction) vs ddpm_step (+ the 8 B / token copy that refills its MASKs, timed apart)."""
    from esmdiff_amd import _native as N
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine
    from esmdiff_amd.weights import random_init_state_dict
    eng = Engine(TINY, random_init_state_dict(TINY, seed=1), max_batch=B, max_len=L)
    lib, h = eng._lib, eng._h
    g = torch.Generator().manual_seed(0)
    ld = 4104
    logits = (torch.randn(B, L, ld, generator=g) * 0.6).cuda()
    xt = torch.full((B, L), MASK, dtype=torch.int64, device="cuda")
    x0 = torch.randint(0, 4096, (B, L), generator=g).cuda()
    w = (-torch.rand(B, generator=g)).cuda()
    xs = xt.clone()
    ssum = torch.empty(B, dtype=torch.float32, device="cuda")
    scnt = torch.empty(B, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = N.Rng(1, 0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def rows():
        N.check(lib.esmdiff_nelbo_rows(h, P(logits), ld, P(xt), P(x0), P(w), None, None, P(ssum), P(scnt), B, L, st), h)

    def ddpm():
        xs.copy_(xt)      # the step consumes its MASKs: refill (timed apart below and subtracted)
        N.check(lib.esmdiff_ddpm_step(h, P(xs), P(logits), ld, 0.9, 0.8, 0, None, ctypes.byref(rng), 3, B, L, st), h)

    tr, td = alternate(rows, ddpm, iters, rounds)
    tc = [_timed(lambda: xs.copy_(xt), iters) for _ in range(5)]
    eng.close()
    copy = statistics.median(tc)
    out = {"B": B, "L": L, "masked_rows": B * L, "logit_bytes": B * L * 4101 * 4,
           "nelbo_rows_ms": statistics.median(tr), "nelbo_rows_ms_min_max": [min(tr), max(tr)],
           "ddpm_step_ms": statistics.median(td) - copy, "ddpm_step_with_refill_ms_min_max": [min(td), max(td)], "refill_copy_ms": copy}
    out["nelbo_rows_GBps"] = out["logit_bytes"] / (out["nelbo_rows_ms"] * 1e-3) / 1e9
    out["check_rows_not_slower_than_ddpm_step"] = bool(out["nelbo_rows_ms"] <= out["ddpm_step_ms"])
    return out


def measure_engine(precision, ddpm_step_ms, B=100, L=258, rounds=5):
    from esmdiff_amd import _native as N
    from esmdiff_amd import nelbo as NL
    from esmdiff_amd.config import ESM3_OPEN
    from esmdiff_amd.model import random_init_model
    from esmdiff_amd.schedule import timestep_embedding
    m = random_init_model(ESM3_OPEN, seed=0, max_batch=B, max_len=L, precision=precision)
    e = m.net
    lib, h = e._lib, e._h
    g = torch.Generator().manual_seed(1)
    seq = torch.randint(4, 24, (B, L), generator=g).cuda()
    x0 = torch.randint(0, 4096, (B, L), generator=g).cuda()
    xt = torch.full((B, L), MASK, dtype=torch.int64, device="cuda")
    sc = NL.step_scalars(m, NL.sample_t(m, B, torch.rand(B, generator=g)))
    tf = e.conditioning_rows(timestep_embedding(sc["conditioning"], m.cfg.freq_dim)).cuda().contiguous()
    mc = torch.ones(B, device="cuda")          # move chance 1: every row MASK, the scoring kernel's worst case
    wt = sc["weight"].cuda()
    si = torch.arange(B, dtype=torch.int64, device="cuda")
    dr = torch.zeros(B, dtype=torch.int32, device="cuda")
    ssum = torch.empty(B, dtype=torch.float32, device="cuda")
    scnt = torch.empty(B, dtype=torch.int32, device="cuda")
    buf = torch.empty(B, L, e.ld_logits, dtype=torch.float32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def ev():
        N.check(lib.esmdiff_nelbo_eval(h, P(seq), P(x0), P(tf), P(mc), P(wt), None, None, 1, P(si), P(dr), None, 0, P(ssum), P(scnt), None,
                                       B, L, st), h)

    def fw():
        N.check(lib.esmdiff_forward_logits_sigmas(h, P(seq), P(xt), P(tf), P(buf), e.ld_logits, B, L, st), h)

    te, tfw = alternate(ev, fw, 10 if precision == "bf16" else 4, rounds)
    assert int(scnt.sum()) == B * L
    e.close()
    ev_ms, fw_ms = statistics.median(te), statistics.median(tfw)
    out = {"nelbo_eval_ms": ev_ms, "forward_sigmas_ms": fw_ms, "difference_ms": ev_ms - fw_ms, "allowed_difference_ms": ddpm_step_ms + 0.05 * fw_ms,
           "nelbo_eval_ms_all": te, "forward_sigmas_ms_all": tfw, "pairs_per_s": B / (ev_ms * 1e-3)}
    out["check_difference_is_the_two_small_kernels"] = bool(out["difference_ms"] <= out["allowed_difference_ms"])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=100)
    ap.add_argument("--L", type=int, default=258)
    ap.add_argument("--skip-engines", action="store_true")
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("measure_nelbo needs an MI355X: nothing is measured without one")
    out = {"kernels": measure_kernels(a.B, a.L)}
    print(json.dumps(out["kernels"]), flush=True)
    ok = out["kernels"]["check_rows_not_slower_than_ddpm_step"]
    if not a.skip_engines:
        for precision in ("bf16", "f32_split"):
            out[precision] = measure_engine(precision, out["kernels"]["ddpm_step_ms"], a.B, a.L)
            print(json.dumps({precision: out[precision]}), flush=True)
            ok = ok and out[precision]["check_difference_is_the_two_small_kernels"]
            torch.cuda.empty_cache()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1))
    print("CHECKS", "PASS" if ok else "FAIL", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
