"""The caller's-stream contract of esmdiff_kmeans_assign, esmdiff_kmeans_step and esmdiff_transition_counts (csrc/msm.hip) through
esmdiff_amd/pairs.py: on a delayed non-blocking stream against the null stream the outputs are bit-equal and the call has synchronised
the stream, as the other entries of the layer do (tests/stream_order.py).  The step is two kernels a round that hand the chunk sums to
one another through the scratch, and it runs three rounds here (three chunks, one slot): a launch on another stream would read the
stale run's partials.  The transition counts are a check pass, a read-back, a memset and a counting kernel.

A module of its own, named so that it is collected AFTER tests/test_gpu_stream_order.py (test_gpu_states.py would sort before it): that
module's planted cases need its side stream to run beside the null stream, and every module's Clock takes one more stream from torch's
pool (tests/test_gpu_stream_sasa.py tells the story).  Nothing here needs two streams to overlap: the entries wait for their stream."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clock():
    from tests.stream_order import Clock
    return Clock()


@pytest.mark.parametrize("name", ["kmeans_assign", "kmeans_step", "transition_counts", "transition_counts_global"])
def test_entries_work_on_the_callers_stream(clock, name):
    """On a delayed non-blocking stream against the null stream: bit-equal outputs, and the call has synchronised the stream."""
    import torch
    from esmdiff_amd import pairs
    from esmdiff_amd import _native as N
    from tests.stream_order import run_both
    gen = lambda seed: torch.Generator().manual_seed(seed)
    n, d, k = 2 * N.KMEANS_FRAME_CHUNK + 300, 3, N.KMEANS_CENTRE_TILE + 9       # three chunks of frames, two tiles of centres
    frames = lambda s: torch.randn(n, d, generator=gen(1 + s), dtype=torch.float64) * 2.0
    centres = lambda s: torch.randn(k, d, generator=gen(5 + s), dtype=torch.float64) * 2.0
    m = N.TRANSITION_FRAME_CHUNK + 500                                           # two workgroups of pairs
    labels = lambda s, states: [torch.randint(-1, states, (m,), generator=gen(9 + s), dtype=torch.int32)]
    big = N.TRANSITION_LDS_MAX_K + 3
    mk, call = {
        "kmeans_assign": (lambda s: [frames(s), centres(s)], lambda b: pairs.kmeans_assign(b[0], b[1])),
        "kmeans_step": (lambda s: [frames(s), centres(s)], lambda b: pairs.kmeans_step(b[0], b[1], slots=1)),
        "transition_counts": (lambda s: labels(s, 40), lambda b: pairs.transition_counts(b[0], 40, 7)),
        "transition_counts_global": (lambda s: labels(s, big), lambda b: pairs.transition_counts(b[0], big, 7)),
    }[name]
    fresh, stale = [t.cuda() for t in mk(0)], [t.cuda() for t in mk(1)]
    rep = run_both(clock, name, lambda: fresh, lambda: stale, call)
    print(f"MEASURED stream order {rep.name}: host return {rep.host_ms:.3f} ms, delay {rep.delay_ms:.0f} ms, "
          f"busy_on_return {rep.busy_on_return}, mismatches {rep.mismatches}")
    assert rep.ok, (rep.name, rep.mismatches)
    assert rep.busy_on_return is False, (rep.name, "the entry synchronises its stream")
