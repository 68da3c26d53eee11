"""The caller's-stream contract of esmdiff_flex_transforms (csrc/flex.hip), esmdiff_aligned_moments and esmdiff_aligned_project
(csrc/aligned.hip) through esmdiff_amd/pairs.py: on a delayed non-blocking stream against the null stream the outputs are bit-equal and
the call has synchronised the stream, as the other entries of the layer do (tests/stream_order.py).  The moments entry is several
kernels that hand the chunk sums to one another through the scratch, and it runs more than one round here: a launch on another stream
would read the stale run's.

A module of its own, named so that it is collected AFTER tests/test_gpu_stream_order.py (test_gpu_aligned.py, or a
test_gpu_stream_aligned.py, would sort before it):
that module's planted cases need its side stream to run beside the null stream, and every module's Clock takes one more stream from
torch's pool (tests/test_gpu_stream_sasa.py tells the story).  Nothing here needs two streams to overlap: the entries wait for their
stream."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clock():
    from tests.stream_order import Clock
    return Clock()


@pytest.mark.parametrize("name", ["flex_transforms", "aligned_moments", "aligned_moments_raw", "aligned_project"])
def test_entries_work_on_the_callers_stream(clock, name):
    """On a delayed non-blocking stream against the null stream: bit-equal outputs, and the call has synchronised the stream."""
    import torch
    from esmdiff_amd import _native as N
    from esmdiff_amd import pairs
    from tests.stream_order import run_both
    gen = lambda seed: torch.Generator().manual_seed(seed)
    n, L = 2 * N.ALIGNED_FRAME_CHUNK + 30, 9               # three chunks of frames; one slot of scratch: three rounds
    D = 3 * L
    chain = lambda k: torch.cumsum(torch.randn(n, L, 3, generator=gen(1 + k), dtype=torch.float64) * 2.2, 1) + 40.0
    vec = lambda k, *shape: torch.randn(*shape, generator=gen(5 + k), dtype=torch.float64)

    def rows(k):                                            # rotations about z with translations: proper transforms without a fit
        a, T = vec(k, n), torch.zeros(n, 12, dtype=torch.float64)
        T[:, 0], T[:, 1], T[:, 3], T[:, 4], T[:, 8] = torch.cos(a), -torch.sin(a), torch.sin(a), torch.cos(a), 1.0
        T[:, 9:] = vec(k + 1, n, 3) * 20.0
        return T
    use = lambda k: (torch.rand(n, generator=gen(9 + k)) < 0.9).to(torch.uint8)
    mk, call = {
        "flex_transforms": (lambda k: [chain(k), chain(k + 2)[0].contiguous()], lambda b: pairs.flex_transforms(b[0], None, b[1], None)),
        "aligned_moments": (lambda k: [chain(k), rows(k), use(k), vec(k, D) + 40.0], lambda b: pairs.aligned_moments(b[0], b[1], b[2], b[3], slots=1)),
        "aligned_moments_raw": (lambda k: [chain(k), vec(k, D) + 40.0], lambda b: pairs.aligned_moments(b[0], None, None, b[1], slots=2)),
        "aligned_project": (lambda k: [chain(k), rows(k), vec(k, D) + 40.0, vec(k, D, 3)], lambda b: pairs.aligned_project(b[0], b[1], b[2], b[3])),
    }[name]
    fresh, stale = [t.cuda() for t in mk(0)], [t.cuda() for t in mk(1)]
    rep = run_both(clock, name, lambda: fresh, lambda: stale, call)
    print(f"MEASURED stream order {rep.name}: host return {rep.host_ms:.3f} ms, delay {rep.delay_ms:.0f} ms, "
          f"busy_on_return {rep.busy_on_return}, mismatches {rep.mismatches}")
    assert rep.ok, (rep.name, rep.mismatches)
    assert rep.busy_on_return is False, (rep.name, "the entry synchronises its stream")
