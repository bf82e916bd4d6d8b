"""The two-batch pipeline of FecEngine::process_blocks (SDHIP_FEC_OVERLAP, default on: batch i+1's Viterbi forward pass is queued before the
host turns to batch i's traceback / BER / deframer / RS) against the serial order (SDHIP_FEC_OVERLAP=0), in one process, byte for byte:
the CADUs, the frame count, FecStats and the per-block taps. The serial order is what the other FEC GPU tests hold against the oracle.

Streams: synthetic MetOp, GOES and NPP (tests/util.py on satdump_amd.synth); a GOES stream with a stretch of noise in which the Viterbi lock
FSM drops to IDLE and re-locks inside a call (a batch issued ahead is discarded); a MetOp stream with a run of frames without a sync marker,
on which the decoder stays locked while the deframer does not, until the module's watchdog resets the decoder (the run is cut short). Each
with the default batch size (one batch per call at these sizes) and with a batch of a few blocks, so that a call crosses dozens of batch
boundaries -- every one of them a start state guessed ahead and checked afterwards."""
import numpy as np
import pytest

from satdump_amd import synth
from tests import util

pytestmark = pytest.mark.gpu

# frames per stream and blocks per batch of the "small batch" runs (the host-twin collection of these tests shrinks them)
SIZES = {"frames": 600, "batch": 12}
# noise of the soft symbols (synth.soft_from_symbols): the decoders lock, the Viterbi corrects errors in every block, RS in most frames
SIGMA = {"goes": 36, "npp": 40, "metop": 35}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    return torch


@pytest.fixture(scope="module")
def capi():
    from satdump_amd import capi as c
    c.lib()
    return c


def _stream(capi, name):
    """(decoder configuration, int8 soft stream, soft bytes per Viterbi block)"""
    nf = SIZES["frames"]
    if name in ("goes", "goes_noise"):
        spec, cadus, plain, syms = util.goes_case(nframes=nf, seed=21)
        soft = synth.soft_from_symbols(syms, spec, sigma=SIGMA["goes"], seed=5)
        cfg = capi.fec_cfg(constellation="bpsk", nrzm=1, rs_i=4, rs_type=capi.RS223, rs_usecheck=1)
        if name == "goes_noise":
            # 40 blocks of noise from block nb/2 + 3 on (not a multiple of any batch size used here): more than viterbi_outsync_after bad blocks in a row
            soft = soft.copy()
            a = (len(soft) // 8192 // 2 + 3) * 8192 + 1234
            soft[a:a + 40 * 8192] = np.random.default_rng(77).integers(-127, 128, 40 * 8192).astype(np.int8)
        return cfg, soft, 8192
    if name == "npp":
        spec, cadus, plain, syms = util.npp_case(nframes=nf, seed=22)
        soft = synth.soft_from_symbols(syms, spec, sigma=SIGMA["npp"], seed=6)
        return capi.fec_cfg(constellation="qpsk", nrzm=1, rs_i=4, rs_type=capi.RS223, rs_usecheck=1), soft, 8192
    assert name in ("metop", "metop_watchdog")
    spec, cadus, plain, syms = util.metop_case(nframes=nf, seed=23)
    if name == "metop_watchdog":
        # 40 frames in the middle without their sync marker: the code words are valid (the Viterbi stays locked), the deframer falls to NOSYNC and stays
        # there for more than 10 decoder blocks
        cadus = cadus.copy()
        cadus[nf // 2:nf // 2 + 40, :4] = np.random.default_rng(78).integers(0, 256, (40, 4)).astype(np.uint8)
        syms = synth.frames_to_symbols(cadus, spec)
    soft = synth.soft_from_symbols(syms, spec, sigma=SIGMA["metop"], seed=7)
    return capi.fec_cfg(decoder=capi.DEC_METOP_AHRPT, viterbi_ber_thresold=0.17, viterbi_outsync_after=5), soft, 16384


def _stats_tuple(st):
    return (st.soft_in, st.blocks, st.bits_decoded, st.frames_deframed, st.frames_out, np.float32(st.viterbi_ber).view(np.uint32).item(), st.viterbi_lock,
            st.deframer_state, tuple(st.rs_errors), st.vit_respec, st.tb_respec, st.watchdog_events)


def _decode(torch, capi, monkeypatch, cfg, soft, overlap, batch, bounds=None):
    """The stream through one decoder, in the calls `bounds` cuts it into. Everything a call hands back, per call."""
    monkeypatch.setenv("SDHIP_FEC_OVERLAP", str(overlap))
    if batch:
        monkeypatch.setenv("SDHIP_FEC_BATCH", str(batch))  # read when the decoder is created
    else:
        monkeypatch.delenv("SDHIP_FEC_BATCH", raising=False)
    dec = capi.FecDecoder(cfg)
    d_soft = torch.from_numpy(np.ascontiguousarray(soft)).cuda()
    cap = len(soft) // 4096 + 16
    bounds = bounds or [0, len(soft)]
    calls = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        d_out = torch.zeros((cap, dec.cadu_bytes), dtype=torch.uint8, device="cuda")
        n = dec.process_dev(d_soft.data_ptr() + a, b - a, d_out.data_ptr(), cap)
        ber, state = dec.block_taps()
        calls.append(dict(n=n, cadu=d_out[:n].cpu().numpy().copy(), ber=np.array(ber, dtype=np.float32).view(np.uint32).copy(), state=np.array(state).copy(),
                          stats=_stats_tuple(dec.stats())))
    dec.close()
    return calls


def _assert_same(serial, piped):
    assert len(serial) == len(piped)
    for k, (s, p) in enumerate(zip(serial, piped)):
        assert s["n"] == p["n"], f"call {k}: frame count {p['n']} with the pipeline, {s['n']} without"
        assert s["cadu"].shape == p["cadu"].shape and np.array_equal(s["cadu"], p["cadu"]), f"call {k}: CADUs differ"
        assert np.array_equal(s["state"], p["state"]), f"call {k}: per-block decoder state differs"
        assert np.array_equal(s["ber"], p["ber"]), f"call {k}: per-block BER differs"
        assert s["stats"] == p["stats"], f"call {k}: FecStats differ: {p['stats']} with the pipeline, {s['stats']} without"


@pytest.mark.parametrize("small_batch", [False, True], ids=["default_batch", "small_batch"])
@pytest.mark.parametrize("name", ["metop", "goes", "npp"])
def test_pipeline_equals_serial_order(torch_cuda, capi, monkeypatch, name, small_batch):
    """A locked stream: every batch but the first of a call is issued ahead; nothing may change."""
    cfg, soft, B = _stream(capi, name)
    batch = SIZES["batch"] if small_batch else 0
    serial = _decode(torch_cuda, capi, monkeypatch, cfg, soft, 0, batch)
    piped = _decode(torch_cuda, capi, monkeypatch, cfg, soft, 1, batch)
    _assert_same(serial, piped)
    nblk = len(soft) // B
    assert serial[0]["stats"][1] == nblk and len(serial[0]["state"]) == nblk
    assert serial[0]["n"] > SIZES["frames"] * 3 // 4, "the stream should decode: the comparison is about frames, not about their absence"
    if small_batch:
        assert nblk // batch >= (24 if SIZES["frames"] >= 400 else 4), "too few batch boundaries for this test to mean anything"


@pytest.mark.parametrize("small_batch", [False, True], ids=["default_batch", "small_batch"])
def test_pipeline_uneven_calls(torch_cuda, capi, monkeypatch, small_batch):
    """One stream in several process_dev calls of uneven size (partial blocks carried from call to call, a call of one block, an empty one)."""
    cfg, soft, B = _stream(capi, "metop")
    n = len(soft)
    bounds = [0, 1000, 1000, B * 3 + 17, B * 4 + 17, B * 41, B * 41 + 5, (n // B) * B // 2 + 333, n]
    assert bounds == sorted(bounds)
    batch = SIZES["batch"] if small_batch else 0
    serial = _decode(torch_cuda, capi, monkeypatch, cfg, soft, 0, batch, bounds)
    piped = _decode(torch_cuda, capi, monkeypatch, cfg, soft, 1, batch, bounds)
    _assert_same(serial, piped)
    whole = _decode(torch_cuda, capi, monkeypatch, cfg, soft, 1, batch)
    assert np.array_equal(np.concatenate([c["cadu"] for c in piped]), whole[0]["cadu"])
    assert sum(c["n"] for c in piped) > SIZES["frames"] * 3 // 4


@pytest.mark.parametrize("small_batch", [False, True], ids=["default_batch", "small_batch"])
def test_pipeline_lock_loss_discards_the_batch_issued_ahead(torch_cuda, capi, monkeypatch, small_batch):
    """Noise inside a call: the lock FSM gives up in the middle of a batch (accepted < n), the batch issued ahead is dropped, the search runs block
    by block, the decoder re-locks and the pipeline starts again -- all inside one call."""
    cfg, soft, B = _stream(capi, "goes_noise")
    batch = SIZES["batch"] if small_batch else 0
    serial = _decode(torch_cuda, capi, monkeypatch, cfg, soft, 0, batch)
    state = serial[0]["state"]
    idle = np.flatnonzero(state == 0)
    # (the premise of the test, on the serial order: the noise does drive the decoder to IDLE, and it locks again behind it)
    assert len(idle) >= 10 and idle[0] > 10 and (state[idle[-1] + 1:] == 1).all() and idle[-1] + 10 < len(state), "the noise stretch did not unlock the decoder inside the call"
    piped = _decode(torch_cuda, capi, monkeypatch, cfg, soft, 1, batch)
    _assert_same(serial, piped)
    assert serial[0]["n"] > SIZES["frames"] // 2


@pytest.mark.parametrize("small_batch", [False, True], ids=["default_batch", "small_batch"])
def test_pipeline_watchdog_cuts_the_run(torch_cuda, capi, monkeypatch, small_batch):
    """MetOp: ten decoder blocks in a row that end with the deframer in NOSYNC reset the Viterbi decoder; the rest of the batch (used < accepted) and
    the batch issued ahead are decoded again after the new lock search."""
    cfg, soft, B = _stream(capi, "metop_watchdog")
    batch = SIZES["batch"] if small_batch else 0
    serial = _decode(torch_cuda, capi, monkeypatch, cfg, soft, 0, batch)
    assert serial[0]["stats"][-1] >= 1, "the watchdog did not fire: the stream does not cover what this test is for"
    piped = _decode(torch_cuda, capi, monkeypatch, cfg, soft, 1, batch)
    _assert_same(serial, piped)
    assert serial[0]["n"] > SIZES["frames"] // 2
