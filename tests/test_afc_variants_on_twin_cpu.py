"""tests/test_afc_variants_gpu.py, the very same test functions, collected a second time against the HOST TWIN of the engine (tests/emu) and the fixtures
recorded through it on the parent commit (tests/golden/afc_parent/twin_*.npz: the twin's sqrtf is not v_sqrt_f32, so they are a set of their own). Runs in the
CPU suite (-m "not gpu"); proves that the variants' source computes what the parent's did, not the GPU build -- that stays with -m gpu."""
import pytest

from tests import afc_variants_util as U
from tests import test_afc_variants_gpu as G
from tests.emu import fake_torch


@pytest.fixture(scope="module")
def torch_cuda():
    return fake_torch


@pytest.fixture(scope="module")
def capi():
    m = U.twin_capi()
    if m is None:
        pytest.skip("no host clang++ to build the twin with")
    return m


@pytest.fixture(scope="module")
def inputs():
    return {n: U.signal(c) for n, c in U.CASES.items()}


@pytest.fixture(autouse=True)
def _twin_fixtures(monkeypatch):
    monkeypatch.setattr(G, "BACKEND", "twin")


def _plain(f):
    """the function without its gpu mark (parametrisation kept)"""
    import functools
    import inspect

    def g(*a, **kw):
        return f(*a, **kw)
    g = functools.wraps(f)(g)
    g.__signature__ = inspect.signature(f)
    g.pytestmark = [m for m in getattr(f, "pytestmark", []) if m.name != "gpu"]
    return g


test_psk_demod_equals_the_parent = _plain(G.test_psk_demod_equals_the_parent)
test_per_lane_path_equals_the_parent = _plain(G.test_per_lane_path_equals_the_parent)
test_agc_blocks_equal_the_parent = _plain(G.test_agc_blocks_equal_the_parent)
test_exact_mode_equals_the_oracle = _plain(G.test_exact_mode_equals_the_oracle)
