"""The GPU parity tests of ccsds_turbo_decoder (tests/test_ccsds_turbo_gpu.py), the very same test functions, collected a second time against the HOST TWIN of the
engine (tests/emu), the way tests/test_ccsds_ldpc_on_twin_cpu.py collects the LDPC decoder's: `torch_cuda` is a numpy stand-in, `capi` the ctypes binding opened on
the twin. Runs in the CPU suite (-m "not gpu"); proves host logic and arithmetic, not the GPU build -- that stays with -m gpu.

The twin links the libm the fixtures were recorded with, so here the a-priori arrays of the BCJR unit are held BIT FOR BIT (BACKEND = "twin"): a difference is an
operation in another order, not a rounding of exp / log.

Left to the GPU suite, to keep the CPU suite short: the three-call and ragged-call runs of the rate 1/3 and 1/4 streams, the second host push / pull run, the
unit decodes of bases 892 and 1115 (the emulated recursion takes a fibre switch per lane and trellis step), the three-call runs of the five-frame streams of
the longer blocks and the ragged runs of two of them, and the base 1115 codewords of test_decode_combos."""
import pytest

from tests import test_ccsds_turbo_gpu as G
from tests import test_ccsds_turbo_waterfall_gpu as W
from tests.emu import fake_torch
from tests.test_dvbs2_on_twin_cpu import capi  # noqa: F401  (fixture: the twin's binding)
from tests.test_fsk_on_twin_cpu import _plain


@pytest.fixture(scope="module")
def torch_cuda():
    return fake_torch


@pytest.fixture(autouse=True)
def _twin(monkeypatch):
    monkeypatch.setattr(G, "BACKEND", "twin")


test_defaults = G.test_defaults
test_refusals = _plain(G.test_refusals)
test_unit_correlator_bit_exact = _plain(G.test_unit_correlator_bit_exact)
test_bcjr_unit = _plain(G.test_bcjr_unit)
test_unit_decode_rails = _plain(G.test_unit_decode_rails)
test_stream_one_call = _plain(G.test_stream_one_call)
test_statistics_inside_a_slide = _plain(G.test_statistics_inside_a_slide)


@pytest.mark.parametrize("iterations", [1, 2])
def test_unit_decode(torch_cuda, capi, iterations):
    G.test_unit_decode(torch_cuda, capi, "dec_b446_r13", "1/3", 446, iterations)


@pytest.mark.parametrize("name", ["r12_b223", "r16_b223"])
def test_stream_three_calls(torch_cuda, capi, name):
    G.test_stream_three_calls(torch_cuda, capi, name)


@pytest.mark.parametrize("name", ["r12_b223", "r16_b223", "r13_b446"])
def test_stream_ragged_calls(torch_cuda, capi, name):
    G.test_stream_ragged_calls(torch_cuda, capi, name)


def test_host_push_pull_path(capi):
    G.test_host_push_pull_path(capi, "r13_b223")


# ---- inside the waterfall (tests/test_ccsds_turbo_waterfall_gpu.py): here every (frame, iteration) pair and every recorded array is held bit for bit
test_decode_every_iteration = _plain(W.test_decode_every_iteration)
test_bcjr_passes_late_iterations = _plain(W.test_bcjr_passes_late_iterations)
test_bcjr_batch_is_per_frame = _plain(W.test_bcjr_batch_is_per_frame)
test_unlocked_stream = _plain(W.test_unlocked_stream)
test_stream_needs_its_iterations = _plain(W.test_stream_needs_its_iterations)


@pytest.mark.parametrize("tag,base", [c for c in W.COMBOS if c[1] != 1115])  # (base 1115 stays with the GPU suite, to keep the CPU suite short)
def test_decode_combos(torch_cuda, capi, tag, base):
    W.test_decode_combos(torch_cuda, capi, tag, base)
