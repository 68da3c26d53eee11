"""The caller's-stream contract of esmdiff_sasa_frames and esmdiff_cooccurrence (csrc/sasa.hip) through esmdiff_amd/pairs.py: on a
delayed non-blocking stream against the null stream the outputs are bit-equal and the call has synchronised the stream, as the other
entries of the layer do (tests/stream_order.py).

A module of its own, named so that it is collected AFTER tests/test_gpu_stream_order.py.  That module's planted cases need its side
stream to run beside the null stream.  Every module's Clock takes one more stream from torch's pool, and with the default of four
hardware queues a process opens, the streams share queues in turn: with these tests collected before it (in tests/test_gpu_sasa.py,
one more side stream used ahead of it), test_a_launch_on_the_null_stream_is_reported found its planted null-stream launch running in
order behind the delay — one queue for both — and failed; collected after it, the whole suite passes.  Nothing here needs two streams
to overlap: both entries wait for their stream."""
import numpy as np
import pytest

from tests import sasa_ref as R

pytestmark = pytest.mark.gpu

BACKBONE_R = np.add(R.DEFAULT_RADII, 1.4)


@pytest.fixture(scope="module")
def clock():
    from tests.stream_order import Clock
    return Clock()


@pytest.mark.parametrize("name", ["sasa_frames", "sasa_frames_long", "cooccurrence"])
def test_entries_work_on_the_callers_stream(clock, name):
    """On a delayed non-blocking stream against the null stream: bit-equal outputs, and the call has synchronised the stream."""
    import torch
    from esmdiff_amd import pairs
    from tests.stream_order import run_both
    gen = lambda seed: torch.Generator().manual_seed(seed)
    chain = lambda k, n, L: torch.cumsum(torch.randn(n, L, 1, 3, generator=gen(1 + k), dtype=torch.float64) * 2.2, 1) + \
        torch.randn(n, L, 4, 3, generator=gen(3 + k), dtype=torch.float64)
    radii = lambda L: torch.as_tensor(np.tile(BACKBONE_R, (L, 1)))
    points = torch.as_tensor(R.sphere_points(96))
    flags = lambda k: (torch.rand(200, 70, generator=gen(7 + k)) * 2.3).to(torch.uint8)
    frames = lambda b: tuple(pairs.sasa_frames(b[0], None, b[1], b[2], 0.2).values())
    mk, call = {
        "sasa_frames": (lambda k: [chain(k, 11, 20), radii(20), points], frames),
        "sasa_frames_long": (lambda k: [chain(k, 2, 70), radii(70), points], frames),
        "cooccurrence": (lambda k: [flags(k)], lambda b: pairs.cooccurrence(b[0])),
    }[name]
    fresh, stale = [t.cuda() for t in mk(0)], [t.cuda() for t in mk(1)]
    rep = run_both(clock, name, lambda: fresh, lambda: stale, call)
    print(f"MEASURED stream order {rep.name}: host return {rep.host_ms:.3f} ms, delay {rep.delay_ms:.0f} ms, "
          f"busy_on_return {rep.busy_on_return}, mismatches {rep.mismatches}")
    assert rep.ok, (rep.name, rep.mismatches)
    assert rep.busy_on_return is False, (rep.name, "the entry synchronises its stream")
