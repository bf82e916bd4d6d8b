"""The GPU parity tests of fsk_demod / sdpsk_demod (tests/test_fsk_gpu.py), the very same test functions, collected a second time against the HOST TWIN of the
engine (tests/emu), the way tests/test_demod_gpu_on_twin_cpu.py collects the PSK chain's: `torch_cuda` is a numpy stand-in, `capi` the ctypes binding opened on
the twin, the decoder behind the demodulator (the end-to-end test) the oracle's. Runs in the CPU suite (-m "not gpu"); proves host logic and arithmetic, not
the GPU build -- that stays with -m gpu."""
import pytest

from tests import test_demod_gpu_on_twin_cpu as T
from tests import test_fsk_gpu as G

torch_cuda = T.torch_cuda
capi = T.capi


def _plain(f):
    """the function without its gpu mark (parametrisation kept)"""
    marks = [m for m in getattr(f, "pytestmark", []) if m.name != "gpu"]
    inner = getattr(f, "__wrapped__", f)

    def g(*a, **kw):
        return inner(*a, **kw)
    import functools
    import inspect
    g = functools.wraps(inner)(g)
    g.__signature__ = inspect.signature(inner)
    g.pytestmark = marks
    return g


test_defaults = G.test_defaults
test_single_blocks_bit_exact = _plain(G.test_single_blocks_bit_exact)
test_exact_mode_bit_identical = _plain(G.test_exact_mode_bit_identical)
test_chunk_parallel_mode = _plain(G.test_chunk_parallel_mode)
test_host_push_pull_path = _plain(G.test_host_push_pull_path)
test_empty_and_tiny_calls = _plain(G.test_empty_and_tiny_calls)
test_end_to_end_cadus = _plain(G.test_end_to_end_cadus)
test_noise_only_input = _plain(G.test_noise_only_input)
test_refusals = _plain(G.test_refusals)
