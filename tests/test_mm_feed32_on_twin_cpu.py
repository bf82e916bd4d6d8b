"""tests/test_mm_feed32_gpu.py, the very same test functions, collected a second time against the HOST TWIN of the engine (tests/emu): k_mm's 32-sample
feeds against its 16- and 8-sample feeds in the CPU suite (-m "not gpu"). The twin runs the kernel's own source lane by lane, so what it proves is the source:
the checkpoint rule of a feed of four blocks, the 64-slot ring and its mirror, the switch and the occupancy rule of the default (the twin's runtime reports
8 CUs: 32 blocks). The GPU build stays with -m gpu.

Sabotage, on the twin (a copy of the sources built beside it, EMU_CSRC / EMU_TAG of tests/emu/build.py), 31 cases in all:
  * feed_body's checkpoint rule left at one per 16 samples (`r < 16` for `r < FEED`): a checkpoint that ends the first or second block of a 32-sample feed
    is never taken, so a re-run lane reads a record nobody wrote there. 24 cases fail: the 6 of test_feed32_failed_handoffs_and_checkpoints, the 6 of
    test_feed32_streams_cut_into_calls and 12 of the 14 of test_feed32_bit_identical_to_feed16_and_feed8 (warm-ups of 256 and 512 samples leave re-runs
    in all of them). What passes has no re-run that reads a checkpoint, or compares no bytes: the two single-call cases at 8.571 samples per symbol
    (warm-up 1024), test_the_width_asked_for_is_the_width_that_ran, test_a_launch_of_more_than_four_blocks_per_cu_keeps_16 (64-sample chunks hold no
    checkpoint).
  * the ring left at 32 slots under 32-sample feeds (mm_ring_mm(32) = 32, the static_asserts that refuse it taken out): a window that starts in the feed's
    first block reads samples the feed's last block has overwritten. 27 cases fail: every case that compares bytes; the 4 of
    test_the_width_asked_for_is_the_width_that_ran pass."""
import pytest

from tests import afc_variants_util as U
from tests import test_mm_feed32_gpu as G
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


test_feed32_bit_identical_to_feed16_and_feed8 = _plain(G.test_feed32_bit_identical_to_feed16_and_feed8)
test_feed32_streams_cut_into_calls = _plain(G.test_feed32_streams_cut_into_calls)
test_feed32_failed_handoffs_and_checkpoints = _plain(G.test_feed32_failed_handoffs_and_checkpoints)
test_the_width_asked_for_is_the_width_that_ran = _plain(G.test_the_width_asked_for_is_the_width_that_ran)
test_a_launch_of_more_than_four_blocks_per_cu_keeps_16 = _plain(G.test_a_launch_of_more_than_four_blocks_per_cu_keeps_16)
