"""The caller's-stream contract of esmdiff_lagged_means, esmdiff_lagged_moments and esmdiff_lagged_project (csrc/lagged.hip) through
esmdiff_amd/pairs.py: on a delayed non-blocking stream against the null stream the outputs are bit-equal and the call has synchronised
the stream, as the other entries of the layer do (tests/stream_order.py).  Each entry is several kernels that hand the pair table and
the chunk sums to one another through the scratch, and the moments entry runs more than one round here: a launch on another stream
would read the stale run's.

A module of its own, named so that it is collected AFTER tests/test_gpu_stream_order.py (test_gpu_kinetics.py would sort before it):
that module's planted cases need its side stream to run beside the null stream, and every module's Clock takes one more stream from
torch's pool (tests/test_gpu_stream_sasa.py tells the story).  Nothing here needs two streams to overlap: the entries wait for their
stream."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clock():
    from tests.stream_order import Clock
    return Clock()


@pytest.mark.parametrize("name", ["lagged_means", "lagged_moments", "lagged_moments_features", "lagged_project"])
def test_entries_work_on_the_callers_stream(clock, name):
    """On a delayed non-blocking stream against the null stream: bit-equal outputs, and the call has synchronised the stream."""
    import torch
    from esmdiff_amd import pairs
    from tests.stream_order import run_both
    gen = lambda seed: torch.Generator().manual_seed(seed)
    from esmdiff_amd import _native as N
    n, L, lag = 2 * N.LAGGED_FRAME_CHUNK + 300, 9, 7       # three chunks of frames; one slot of scratch: three rounds
    D = (L - 1) * L // 2
    chain = lambda k: torch.cumsum(torch.randn(n, L, 3, generator=gen(1 + k), dtype=torch.float64) * 2.2, 1)
    vec = lambda k, *shape: torch.randn(*shape, generator=gen(5 + k), dtype=torch.float64)
    mk, call = {
        "lagged_means": (lambda k: [chain(k)], lambda b: pairs.lagged_means(b[0], lag, 1, slots=1)),
        "lagged_moments": (lambda k: [chain(k), vec(k, D) + 8.0], lambda b: pairs.lagged_moments(b[0], lag, b[1], 1, slots=1)),
        "lagged_moments_features": (lambda k: [vec(k, n, 40), vec(k, 40)], lambda b: pairs.lagged_moments(b[0], lag, b[1], 0, slots=2)),
        "lagged_project": (lambda k: [chain(k), vec(k, D) + 8.0, vec(k, D, 3)], lambda b: pairs.lagged_project(b[0], b[1], b[2], 1)),
    }[name]
    fresh, stale = [t.cuda() for t in mk(0)], [t.cuda() for t in mk(1)]
    rep = run_both(clock, name, lambda: fresh, lambda: stale, call)
    print(f"MEASURED stream order {rep.name}: host return {rep.host_ms:.3f} ms, delay {rep.delay_ms:.0f} ms, "
          f"busy_on_return {rep.busy_on_return}, mismatches {rep.mismatches}")
    assert rep.ok, (rep.name, rep.mismatches)
    assert rep.busy_on_return is False, (rep.name, "the entry synchronises its stream")
