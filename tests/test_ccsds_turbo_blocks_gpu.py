"""What a ccsds_turbo_decoder handle finds in its blocks, in the pattern of tests/test_block_contents_gpu.py: the block pool is on, every fresh block is handed out
filled with 0xFF bytes (as doubles NaN, as descriptors and flags anything but the zero of a fresh page), a first handle decodes ANOTHER stream (rate 1/6: larger
buffers throughout) and is destroyed, and a second handle, built from the blocks it left, must still produce the rate 1/2 fixture bit for bit in three calls.
Guards what the kernels assume of memory nobody wrote: the recursions' first columns (the backward array's last one), the a-priori arrays in front of the first
pass, the pending-read buffer across calls, the slide's pending descriptor."""
import os

import pytest

from tests import test_block_contents_gpu as B
from tests import test_ccsds_turbo_gpu as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    torch.zeros(1, device="cuda")
    return torch


@pytest.fixture(scope="module")
def capi(torch_cuda):
    from satdump_amd import capi as c
    c.lib()
    return c


def test_second_handle_on_filled_and_recycled_blocks(torch_cuda, capi):
    first, second = G._golden("r16_b223"), G._golden("r12_b223")
    with B._clean_state(capi):
        os.environ["SDHIP_ALLOC_FILL"] = "255"
        capi.pool_enable(True)
        s0 = capi.pool_stats()
        n = len(first["soft"])
        G._check(first, *G._run(torch_cuda, capi, first, [0, n // 2 + 33, n]))
        s1 = capi.pool_stats()
        assert s1.filled - s0.filled == s1.dev_fresh + s1.pin_fresh - s0.dev_fresh - s0.pin_fresh > 0, "no block was handed out filled"
        assert s1.dev_parked > 0 and s1.dev_parked_bytes > 0, "handle 1 parked nothing"
        n = len(second["soft"])
        out, descs, st = G._run(torch_cuda, capi, second, [0, n // 3 + 17, 2 * n // 3 + 401, n])
        s2 = capi.pool_stats()
        assert s2.dev_recycled - s1.dev_recycled > 0, "handle 2 recycled no device block: nothing was tested"
        G._check(second, out, descs, st)
