"""The GPU parity tests of ccsds_ldpc_decoder (tests/test_ccsds_ldpc_gpu.py), the very same test functions, collected a second time against the HOST TWIN of the
engine (tests/emu), the way tests/test_fsk_on_twin_cpu.py collects the real-valued demodulators': `torch_cuda` is a numpy stand-in, `capi` the ctypes binding
opened on the twin. Runs in the CPU suite (-m "not gpu"); proves host logic and arithmetic, not the GPU build -- that stays with -m gpu.

Left to the GPU suite: the three-call and ragged-call runs of the two 32-frame streams (a minute each on the emulated decoder kernel; their one-call runs, and the
cut runs of the BPSK and noise streams, are here), the host push / pull run of the direct stream, and 25 iterations of the unit decode."""
import pytest

from tests import test_ccsds_ldpc_gpu as G
from tests.emu import fake_torch
from tests.test_dvbs2_on_twin_cpu import capi  # noqa: F401  (fixture: the twin's binding)
from tests.test_fsk_on_twin_cpu import _plain

SHORT = ["r78_bpsk", "r78_noise"]


@pytest.fixture(scope="module")
def torch_cuda():
    return fake_torch


test_defaults = G.test_defaults
test_unit_decode_rails = _plain(G.test_unit_decode_rails)
test_unit_correlator_bit_exact = _plain(G.test_unit_correlator_bit_exact)
test_stream_one_call = _plain(G.test_stream_one_call)
test_noise_stream_terminates = _plain(G.test_noise_stream_terminates)
test_level_schedule = _plain(G.test_level_schedule)
test_statistics_inside_a_slide = _plain(G.test_statistics_inside_a_slide)
test_generic_row_list_decode = _plain(G.test_generic_row_list_decode)
test_refusals = _plain(G.test_refusals)


@pytest.mark.parametrize("iterations", [1, 10])
def test_unit_decode_bit_exact(torch_cuda, capi, iterations):
    G.test_unit_decode_bit_exact(torch_cuda, capi, iterations)


@pytest.mark.parametrize("name", SHORT + G.SHORT_RAILS)
def test_stream_three_calls(torch_cuda, capi, name):
    G.test_stream_three_calls(torch_cuda, capi, name)


@pytest.mark.parametrize("name", SHORT)
def test_stream_ragged_calls(torch_cuda, capi, name):
    G.test_stream_ragged_calls(torch_cuda, capi, name)


def test_host_push_pull_path(capi):
    G.test_host_push_pull_path(capi, "r78_oqpsk_internal")
