"""The caller's-stream contract of esmdiff_rmsd_prepare and esmdiff_rmsd_nearest (csrc/rmsd_nn.hip) through esmdiff_amd/pairs.py: on a
delayed non-blocking stream against the null stream the outputs are bit-equal and the call has synchronised the stream, as the other
entries of the layer do (tests/stream_order.py).  The nearest entry is an init kernel, then two kernels a round that hand the
rectangles' partials to one another through the scratch, then the kernels that write the outputs; it runs two rounds here (two
rectangles, one slot): a launch on another stream would read the stale run's partials or state.

A module of its own, named so that it is collected AFTER tests/test_gpu_stream_order.py (test_gpu_neighbours.py would sort before it):
tests/test_gpu_stream_states.py tells the story."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clock():
    from tests.stream_order import Clock
    return Clock()


@pytest.mark.parametrize("name", ["rmsd_prepare", "rmsd_nearest", "rmsd_nearest_self"])
def test_entries_work_on_the_callers_stream(clock, name):
    import torch
    from esmdiff_amd import pairs
    from esmdiff_amd import _native as N
    from tests.stream_order import run_both
    gen = lambda seed: torch.Generator().manual_seed(seed)
    n, m, L = 40, N.RMSD_NN_RECT + 9, 13                                         # two rectangles; self mode: m frames, three rectangles
    frames = lambda s, k: torch.randn(k, L, 3, generator=gen(3 + s + k), dtype=torch.float64) * 4.0
    sel = torch.ones(L, dtype=torch.uint8)
    sel[2] = 0

    def sides(s, k):
        p = pairs.rmsd_prepare(frames(s, k).cuda(), sel.cuda(), L - 1)
        torch.cuda.synchronize()
        return [p["P"], p["info"], p["use"]]

    side = lambda b: {"P": b[0], "info": b[1], "use": b[2], "n_sel": L - 1}
    kw = dict(cutoffs=(3.0, 6.0), bins=16, width=1.0, slots=1, dense=("msd",))
    mk, call = {
        "rmsd_prepare": (lambda s: [frames(s, m).cuda(), sel.cuda()], lambda b: pairs.rmsd_prepare(b[0], b[1], L - 1)),
        "rmsd_nearest": (lambda s: sides(s, n) + sides(s, m), lambda b: pairs.rmsd_nearest(side(b[:3]), side(b[3:]), **kw)),
        "rmsd_nearest_self": (lambda s: sides(s, m), lambda b: pairs.rmsd_nearest(side(b), None, **kw)),
    }[name]
    fresh, stale = mk(0), mk(1)
    rep = run_both(clock, name, lambda: fresh, lambda: stale, call)
    print(f"MEASURED stream order {rep.name}: host return {rep.host_ms:.3f} ms, delay {rep.delay_ms:.0f} ms, "
          f"busy_on_return {rep.busy_on_return}, mismatches {rep.mismatches}")
    assert rep.ok, (rep.name, rep.mismatches)
    assert rep.busy_on_return is False, (rep.name, "the entry synchronises its stream")
