"""Run one call on the null stream and once more on a delayed non-default stream, and report what differs (a plain helper).

The ABI's first convention (include/esmdiff_hip.h): all work is enqueued on the caller's stream, and no entry waits unless it
says so.  On the null stream neither half can be seen to fail.  Here the same call runs twice:

  * on the null stream, with fresh inputs, synchronised: the reference outputs, and the host time the call took to return;
  * on a torch.cuda.Stream S (non-blocking, so the null stream is not ordered against it) that starts with a device-side delay.
    The input buffers exist beforehand and hold STALE contents — valid data of the same kind, but other data — and are overwritten
    with the fresh values by device-to-device copies on S behind the delay.  Then the call; `busy_on_return` = S still has work
    when the call comes back; then a clone() of every output on S, the consumer that relies on stream order (a joined side
    stream included).  After S.synchronize() the clones are compared with the reference.

Between the two runs the call is made once more on the null stream with the STALE inputs, synchronised: every engine-owned
workspace, and every buffer a multi-kernel entry keeps between its kernels, then holds intermediates of the stale data, not the
reference run's.  Work that goes to another stream than S runs EARLY, while S is still asleep.  A first kernel that does so reads
the stale inputs; an interior kernel, memset or copy that does so (on the null stream, on a side stream that was not forked, or a
main-stream kernel that reads the side half's buffers without the join) reads those stale intermediates; a last kernel's result
is overwritten, or not yet there when the clones are taken.  In each case the answer differs.  What the harness cannot see: a
misplaced launch whose inputs are the same in both runs (weights, tables), and a missing order between two kernels that the device
happens to run in order anyway.  A call that waited shows busy_on_return = False.  The delay is 20 x the host time measured for
that call on the null stream (at least 50 ms), so that a
call that merely returns slowly on a loaded host is not taken for one that waited.

Outputs are compared bit for bit unless a case brings its own comparison.  An output buffer the case passes in holds a sentinel;
one that a wrapper allocates itself cannot (the reference outputs are kept alive until the comparison, so that the allocator
does not hand the delayed run a block that already holds the answer).
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import torch

DELAY_FACTOR = 20
DELAY_FLOOR_MS = 50.0


@dataclass
class Report:
    name: str
    host_ms: float                 # the null-stream call's time to return
    delay_ms: float                # the delay derived from it
    busy_on_return: bool           # S still had work when the delayed call returned
    mismatches: List[str]          # outputs whose clones differ from the reference
    ref: List[torch.Tensor] = field(default_factory=list)
    got: List[torch.Tensor] = field(default_factory=list)

    @property
    def ok(self) -> bool:
        return not self.mismatches


class Clock:
    """One side stream and the spin kernel's cycles per millisecond, measured once with events."""

    def __init__(self):
        self.stream = torch.cuda.Stream()
        torch.cuda._sleep(1_000_000)                      # (loads the kernel)
        torch.cuda.synchronize()
        n = 5_000_000
        for _ in range(2):                                # the second pass spins for about 25 ms whatever the counter's rate
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(n)
            b.record()
            torch.cuda.synchronize()
            self.cycles_per_ms = n / a.elapsed_time(b)
            n = int(25 * self.cycles_per_ms)
        self.reports: List[Report] = []

    def sleep(self, ms: float) -> None:
        torch.cuda._sleep(int(ms * self.cycles_per_ms))

    def worst(self) -> Optional[Report]:
        return max(self.reports, key=lambda r: r.host_ms) if self.reports else None


def _as_list(out) -> List[torch.Tensor]:
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, dict):
        return [v for v in out.values() if isinstance(v, torch.Tensor)]
    return [t for t in out if isinstance(t, torch.Tensor)]


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same shape, dtype and bytes (NaN payloads included)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous(), b.contiguous()
    return bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8))) if a.numel() else True


def _bitwise(i: int, ref: torch.Tensor, got: torch.Tensor) -> Optional[str]:
    if bits_equal(ref, got):
        return None
    if ref.shape != got.shape or ref.dtype != got.dtype:
        return f"output {i}: {tuple(got.shape)} {got.dtype} against {tuple(ref.shape)} {ref.dtype}"
    n = int((ref.contiguous().view(torch.uint8) != got.contiguous().view(torch.uint8)).sum())
    return f"output {i}: {n} of {ref.numel() * ref.element_size()} bytes differ"


def run_both(clock: Clock, name: str, fresh: Callable[[], Sequence[torch.Tensor]], stale: Callable[[], Sequence[torch.Tensor]],
             call: Callable[[List[torch.Tensor]], object], *, compare: Optional[Callable] = None,
             after_return: Optional[Callable[[], None]] = None, outputs: Optional[Callable[[], Sequence[torch.Tensor]]] = None,
             warm: bool = True) -> Report:
    """fresh() / stale(): the case's device buffers — inputs, buffers updated in place, and sentinel-filled outputs it passes in —
    with the fresh and with the stale contents (same shapes and dtypes; fresh() gives the same values every time).
    outputs(): further buffers, appended to the list the call gets, that exist before the delay, hold a sentinel and are NOT
    overwritten on S — for a case that must see what was in an output buffer when the clone was taken.
    call(buffers) makes the call on torch's current stream and returns its output tensor(s).  compare(i, ref, got) -> None or a
    text, instead of the bit-for-bit comparison.  after_return(): run on the host right after the delayed call has returned and
    busy_on_return is noted, before anything else is enqueued (a case uses it to overwrite [host] arrays it handed in).
    warm: one untimed null-stream call first, so that the timed one does not carry a first launch's code loading."""
    S = clock.stream
    keep = []
    extra = (lambda: list(outputs())) if outputs is not None else (lambda: [])
    if warm:
        keep.append(_as_list(call([t.clone() for t in fresh()] + extra())))
        torch.cuda.synchronize()
    args = [t.clone() for t in fresh()] + extra()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call(args)
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    outs = _as_list(out)
    ref = [o.clone() for o in outs]
    keep.append(outs)

    # the same call on the stale data: whatever the delayed run finds in a workspace now comes from other inputs than its own
    keep.append(_as_list(call([t.clone() for t in stale()] + extra())))
    torch.cuda.synchronize()

    bufs = [t.clone() for t in stale()]
    src = [t.clone() for t in fresh()]
    late = extra()
    assert len(bufs) == len(src) and all(b.shape == s.shape and b.dtype == s.dtype for b, s in zip(bufs, src))
    delay_ms = max(DELAY_FLOOR_MS, DELAY_FACTOR * host_ms)
    assert delay_ms >= DELAY_FLOOR_MS and delay_ms >= DELAY_FACTOR * host_ms
    torch.cuda.synchronize()                               # the device is idle
    with torch.cuda.stream(S):
        clock.sleep(delay_ms)
        for b, s in zip(bufs, src):
            b.copy_(s, non_blocking=True)
        out2 = call(bufs + late)
        busy = not S.query()
        if after_return is not None:
            after_return()
        got = [o.clone() for o in _as_list(out2)]
    S.synchronize()
    torch.cuda.synchronize()

    cmp = compare or _bitwise
    mism = [f"{len(got)} outputs against {len(ref)}"] if len(got) != len(ref) else \
        [m for m in (cmp(i, r, g) for i, (r, g) in enumerate(zip(ref, got))) if m]
    rep = Report(name, host_ms, delay_ms, busy, mism, ref, got)
    clock.reports.append(rep)
    del keep
    return rep
