"""GPU: the routes of the projection dispatch are the recorded ones.

Every route of the ladder gives the same bits (the contracts of include/ivl_hip.h), so the suites that compare outputs cannot see a
call that falls to the library GEMM, or to another kernel, by mistake.  tests/routes.py records which entry points each call of a fixed
grid runs; tests/routes_expected.json is that grid recorded once on the commit before the dispatch became one ladder."""
import pytest
import torch

import routes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    return routes.record()


def test_the_grid_is_the_recorded_grid(recorded):
    want = routes.expected()
    assert len(want) > 1000 and set(recorded) == set(want), sorted(set(recorded) ^ set(want))[:10]


def test_every_call_takes_its_recorded_route(recorded):
    want = routes.expected()
    bad = {k: (want[k], got) for k, got in recorded.items() if want.get(k) != got}
    for k, (w, g) in list(bad.items())[:40]:
        print(f"{k}: recorded {w}, now {g}")
    assert not bad, f"{len(bad)} of {len(recorded)} calls changed their route"


def test_the_grid_reaches_every_entry_point_of_the_table():
    """the expectation itself: each of the 21 symbols of ops.ENTRY_POINTS, the m256 kernel and the library path occur in it"""
    from infinitevl_amd import ops
    seen = {s for v in routes.expected().values() for s in v}
    missing = {n for by_fmt in ops.ENTRY_POINTS.values() for n in by_fmt.values()} | {"ivl_linear_m256_fwd", "library"}
    assert not missing - seen, missing - seen
