"""GPU parity tests of the FEC chain (run with -m gpu on an MI355X): every call goes through the C ABI of
libsdhip.so and is compared, bit for bit, with the oracle (the compiled reference when oracle/_ref is present,
else the restatement)."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyref
from satdump_amd import synth
from tests import util

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def orc():
    return pyref.best()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _symbols(rng, F, nb, kind):
    stride = 2 * (F + 6)
    bits = rng.integers(0, 2, nb * F + 64).astype(np.uint8)
    coded = synth.conv_encode(bits)[: nb * 2 * F]
    if kind == "noise":
        soft = rng.integers(-127, 128, nb * 2 * F)
    elif kind == "saturated":  # full-scale symbols: exercises the uint8 metric wrap of the generic ACS kernel
        soft = (coded.astype(np.int64) * 2 - 1) * 127
        flip = rng.random(len(soft)) < 0.04
        soft = np.where(flip, -soft, soft)
    else:
        amp, sig = {"clean": (60, 20), "noisy": (50, 45)}[kind]
        soft = np.clip(np.rint((coded.astype(float) * 2 - 1) * amp + rng.standard_normal(len(coded)) * sig), -127, 127).astype(np.int64)
    u = soft + 127
    u[u == 128] = 127
    if kind == "noisy":
        u[rng.random(len(u)) < 0.1] = 128  # sprinkle erasures
    syms = np.full(nb * stride, 128, dtype=np.uint8)
    for b in range(nb):
        syms[b * stride: b * stride + 2 * F] = u[b * 2 * F:(b + 1) * 2 * F]
    return syms


@pytest.mark.parametrize("F,nb", [(4096, 9), (12288, 4), (1024, 5), (5116, 3), (640, 7)])
@pytest.mark.parametrize("kind", ["clean", "noisy", "noise", "saturated"])
def test_ccdecoder_bit_exact(torch_cuda, capi, orc, F, nb, kind):
    """k_vit_decode == viterbi::CCDecoder::work chained over blocks (cc_decoder.cpp:295-302)."""
    rng = np.random.default_rng(F + nb)
    syms = _symbols(rng, F, nb, kind)
    want = orc.ccdecoder(F, syms)
    d_syms = _dev(torch_cuda, syms)
    d_out = torch_cuda.zeros(nb * F, dtype=torch_cuda.uint8, device="cuda")
    rc = capi.lib().sdhip_op_ccdecoder(0, F, C.c_void_p(d_syms.data_ptr()), nb, C.c_void_p(d_out.data_ptr()))
    assert rc == 0, capi.last_error()
    got = d_out.cpu().numpy()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("seg", [1024, 2048])
@pytest.mark.parametrize("kind", ["noisy", "noise"])
def test_ccdecoder_long_segments(torch_cuda, capi, orc, seg, kind, monkeypatch):
    """The lane-per-segment decoder with 1024 / 2048 trellis steps per lane (what large batches pick: launch_vit_decode2), forced here on
    a small batch through SDHIP_VIT2_SEG: bit-identical to CCDecoder::work like the 512-step default."""
    monkeypatch.setenv("SDHIP_VIT2_SEG", str(seg))
    F, nb = 12288, 5
    rng = np.random.default_rng(seg)
    syms = _symbols(rng, F, nb, kind)
    want = orc.ccdecoder(F, syms)
    d_syms = _dev(torch_cuda, syms)
    d_out = torch_cuda.zeros(nb * F, dtype=torch_cuda.uint8, device="cuda")
    rc = capi.lib().sdhip_op_ccdecoder(0, F, C.c_void_p(d_syms.data_ptr()), nb, C.c_void_p(d_out.data_ptr()))
    assert rc == 0, capi.last_error()
    assert np.array_equal(d_out.cpu().numpy(), want)


@pytest.mark.parametrize("fill", [-1, 0])
def test_rs_decode_bit_exact(torch_cuda, capi, orc, fill):
    """k_rs == ReedSolomon::decode_interlaved incl. the >t failure / miscorrection boundary (decode.c:32-145)."""
    rng = np.random.default_rng(7)
    nfr = 96
    frames = synth.make_cadus(nfr, seed=8, derand=False)
    for f in range(nfr):
        nerr = f % 24
        pos = rng.choice(255, size=nerr, replace=False)
        frames[f, 4 + pos * 4 + (f % 4)] ^= rng.integers(1, 256, size=nerr, dtype=np.uint8)
    want, ewant = orc.rs_decode(frames, fill_bytes=fill)
    d = _dev(torch_cuda, frames)
    d_err = torch_cuda.zeros(nfr * 4, dtype=torch_cuda.int32, device="cuda")
    rc = capi.lib().sdhip_op_rs_decode(0, C.c_void_p(d.data_ptr() + 4), nfr, 1024, 1, 4, capi.RS223, fill, C.c_void_p(d_err.data_ptr()))
    assert rc == 0, capi.last_error()
    assert np.array_equal(d_err.cpu().numpy().reshape(nfr, 4), ewant)
    assert np.array_equal(d.cpu().numpy(), want)
    assert (ewant == -1).any() and (ewant > 8).any()


def _run_dev(torch, capi, cfg, soft, chunks=None):
    dec = capi.FecDecoder(cfg)
    d_soft = _dev(torch, soft)
    cap = len(soft) // 4096 + 16
    outs, bers, states = [], [], []
    bounds = [0, len(soft)] if not chunks else chunks
    for a, b in zip(bounds[:-1], bounds[1:]):
        d_out = torch.zeros((cap, dec.cadu_bytes), dtype=torch.uint8, device="cuda")
        n = dec.process_dev(d_soft.data_ptr() + a, b - a, d_out.data_ptr(), cap)
        outs.append(d_out[:n].cpu().numpy())
        be, st = dec.block_taps()
        bers.append(be)
        states.append(st)
    return np.concatenate(outs), np.concatenate(bers), np.concatenate(states), dec.stats()


@pytest.mark.parametrize("sigma", [15, 30, 45, 60, 90])
@pytest.mark.parametrize("usecheck", [0, 1])
def test_concat_decoder_bpsk(torch_cuda, capi, orc, sigma, usecheck):
    """GOES-HRIT-like (BASELINE config 2 in miniature): BPSK r=1/2 + NRZ-M + RS(255,223) I=4, from clean to unlocked."""
    spec, cadus, plain, syms = util.goes_case(nframes=40, seed=3)
    soft = synth.soft_from_symbols(syms, spec, sigma=sigma, seed=sigma)
    oc = pyref.fec_cfg(constellation=pyref.BPSK, nrzm=1, rs_usecheck=usecheck)
    want = orc.concat_decode(oc, soft)
    cfg = capi.fec_cfg(constellation="bpsk", nrzm=1, rs_i=4, rs_type=capi.RS223, rs_usecheck=usecheck)
    got, ber, state, st = _run_dev(torch_cuda, capi, cfg, soft)
    assert np.array_equal(state, want["state"])
    assert np.array_equal(ber.view(np.uint32), want["ber"].view(np.uint32))
    assert got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"])
    if sigma <= 30:
        assert util.frame_ids(got, plain)[:6] == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("rs_i,usecheck", [(1, 0), (1, 1), (2, 0)])
def test_short_cadus_and_the_fill_bytes_overrun(torch_cuda, capi, orc, rs_i, usecheck):
    """CADUs shorter than half a Viterbi buffer (the 2048 / 2072-bit pipelines): the reference's deframer returns two frames from
    one call, and with rs_fill_bytes = -1 (the module's default) ReedSolomon's interleave loop runs one byte past every codeblock
    (reedsolomon.cpp:145-156): the first rs_i bytes of the NEXT frame come out as the first corrected message byte of each
    codeword. Found by tools/twin/fec_fuzz2.py (seed 8); the output must match byte for byte, sync-marker bytes included."""
    rng = np.random.default_rng(5 + rs_i)
    cadus = synth.make_cadus(24, seed=77 + rs_i, rs_i=rs_i)
    for f in range(len(cadus)):
        for p in rng.choice(cadus.shape[1] - 4, int(rng.choice([0, 0, 3, 12, 40])), replace=False):
            cadus[f, 4 + p] ^= int(rng.integers(1, 256))
    sp = synth.SynthSpec(constellation="bpsk", samplerate=3e6, symbolrate=1e6, nrzm=True, seed=9)
    soft = synth.soft_from_symbols(synth.frames_to_symbols(cadus, sp), sp, sigma=15.0, seed=4)
    soft = np.concatenate([soft, rng.integers(-127, 128, 8192).astype(np.int8)])
    soft = soft[: len(soft) // 8192 * 8192]
    cs = cadus.shape[1] * 8
    assert cs < 4096 or rs_i > 1
    want = orc.concat_decode(pyref.fec_cfg(constellation=pyref.BPSK, nrzm=1, rs_usecheck=usecheck, cadu_size=cs, rs_i=rs_i), soft)
    cfg = capi.fec_cfg(constellation="bpsk", nrzm=1, rs_i=rs_i, rs_type=capi.RS223, rs_usecheck=usecheck, cadu_size=cs)
    got, ber, state, st = _run_dev(torch_cuda, capi, cfg, soft)
    assert got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"]) and len(got) >= 12
    if rs_i == 1:  # the overrun is visible: some frame's first byte is not the sync marker's
        assert np.any(got[:, 0] != 0x1A)


@pytest.mark.parametrize("const,sigma,rot", [("qpsk", 30, 1), ("qpsk", 70, 0), ("oqpsk", 40, 1), ("qpsk", 120, 1)])
def test_concat_decoder_qpsk(torch_cuda, capi, orc, const, sigma, rot):
    """JPSS-HRD-like (BASELINE config 4 in miniature): QPSK r=1/2 + NRZ-M + RS, with a 90 degree rotated stream."""
    spec, cadus, plain, syms = util.npp_case(nframes=40, seed=9)
    soft = synth.soft_from_symbols(syms, spec, sigma=sigma, seed=1)
    if rot:
        s2 = soft.copy()
        s2[0::2], s2[1::2] = soft[1::2], -soft[0::2]
        soft = s2
    oc = pyref.fec_cfg(constellation=getattr(pyref, const.upper()), nrzm=1, rs_usecheck=1)
    want = orc.concat_decode(oc, soft)
    cfg = capi.fec_cfg(constellation=const, nrzm=1, rs_i=4, rs_type=capi.RS223, rs_usecheck=1)
    got, ber, state, st = _run_dev(torch_cuda, capi, cfg, soft)
    assert np.array_equal(state, want["state"])
    assert np.array_equal(ber.view(np.uint32), want["ber"].view(np.uint32))
    assert got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"])


@pytest.mark.parametrize("sigma", [20, 50, 80, 130])
def test_metop_decoder(torch_cuda, capi, orc, sigma):
    """MetOp AHRPT (BASELINE configs 1/3 in miniature): QPSK + punctured r=3/4 + RS, deframer SYNCED=18, all frames written."""
    spec, cadus, plain, syms = util.metop_case(nframes=60, seed=5)
    soft = synth.soft_from_symbols(syms, spec, sigma=sigma, seed=2)
    want = orc.metop_decode(soft)
    cfg = capi.fec_cfg(decoder=capi.DEC_METOP_AHRPT, viterbi_ber_thresold=0.17, viterbi_outsync_after=5)
    got, ber, state, st = _run_dev(torch_cuda, capi, cfg, soft)
    assert np.array_equal(state, want["state"])
    assert np.array_equal(ber.view(np.uint32), want["ber"].view(np.uint32))
    assert got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"])


def test_streaming_chunks_equal_one_shot(torch_cuda, capi, orc):
    """Ragged pushes (partial blocks, empty call) give the same CADUs as one call; also the host push/pull path."""
    spec, cadus, plain, syms = util.goes_case(nframes=30, seed=6)
    soft = synth.soft_from_symbols(syms, spec, sigma=28, seed=3)
    oc = pyref.fec_cfg(constellation=pyref.BPSK, nrzm=1, rs_usecheck=1)
    want = orc.concat_decode(oc, soft)["cadu"]
    cfg = capi.fec_cfg(constellation="bpsk", nrzm=1, rs_i=4, rs_type=capi.RS223, rs_usecheck=1)
    n = len(soft)
    bounds = [0, 1000, 1000, 8192 * 3 + 17, 8192 * 11, 8192 * 11 + 5, n]
    got, _, _, _ = _run_dev(torch_cuda, capi, cfg, soft, chunks=bounds)
    nfull = (n // 8192) * 8192
    assert np.array_equal(got, want)
    dec = capi.FecDecoder(cfg)
    for a, b in zip(bounds[:-1], bounds[1:]):
        dec.push(soft[a:b])
    assert np.array_equal(dec.pull(), want)
    assert nfull > 0


def test_sync_loss_and_inversion(torch_cuda, capi, orc):
    """Deframer corner cases: garbage prefix, dropped symbols mid-stream (bit slip), polarity inversion (non-NRZ-M)."""
    spec, cadus, plain, syms = util.goes_case(nframes=36, seed=12)
    spec.nrzm = False
    syms = synth.frames_to_symbols(cadus, spec)
    soft = synth.soft_from_symbols(syms, spec, sigma=20, seed=4)
    rng = np.random.default_rng(1)
    junk = rng.integers(-60, 60, 5000).astype(np.int8)
    cut = 16384 * 9 + 2 * 777  # drop an even number of soft symbols: the Viterbi stays locked, frames slip
    s2 = np.concatenate([junk, soft[:cut], soft[cut + 2 * 1501:16384 * 20], -soft[16384 * 20:]])
    oc = pyref.fec_cfg(constellation=pyref.BPSK, nrzm=0, rs_usecheck=0)
    want = orc.concat_decode(oc, s2)
    cfg = capi.fec_cfg(constellation="bpsk", nrzm=0, rs_i=4, rs_type=capi.RS223, rs_usecheck=0)
    got, ber, state, st = _run_dev(torch_cuda, capi, cfg, s2)
    assert np.array_equal(state, want["state"])
    assert got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"])
    assert len(got) > 25


@pytest.mark.parametrize("name", [c[0] for c in util.SIMPLE_CASES])
@pytest.mark.parametrize("sigma,usecheck", [(15.0, 1), (28.0, 0)])
def test_simple_psk_decoder(torch_cuda, capi, orc, name, sigma, usecheck):
    """ccsds_simple_psk_decoder on the GPU (bit slicers, one or two deframers, derand, RS) == the reference module loop,
    frame for frame and in the reference's output order (deframer_qpsk's frames of a buffer before the main deframer's)."""
    ck, soft, plain = util.simple_case(name, sigma=sigma, nframes=16)
    ock = dict(ck)
    ock["constellation"] = {"bpsk": pyref.BPSK, "qpsk": pyref.QPSK}[ck["constellation"]]
    want = orc.simple_decode(pyref.fec_cfg(decoder=2, rs_usecheck=usecheck, **ock), soft)
    cfg = capi.fec_cfg(decoder=capi.DEC_SIMPLE_PSK, rs_i=4, rs_type=capi.RS223, rs_usecheck=usecheck, **ck)
    got, _, _, st = _run_dev(torch_cuda, capi, cfg, soft)
    assert st.frames_deframed == want["n_deframed"]
    assert got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"])
    # ragged calls (partial buffers, an empty call) and the host push/pull path give the same stream
    n = len(soft)
    bounds = [0, 1001, 1001, 8192 * 2 + 18, 8192 * 5, 8192 * 5 + 6, n]
    got2, _, _, _ = _run_dev(torch_cuda, capi, cfg, soft, chunks=bounds)
    assert np.array_equal(got2, want["cadu"])
    dec = capi.FecDecoder(cfg)
    for a, b in zip(bounds[:-1], bounds[1:]):
        dec.push(soft[a:b])
    assert np.array_equal(dec.pull(), want["cadu"])


@pytest.mark.parametrize("sigma", [15.0, 40.0, 70.0])
def test_viterbi27(torch_cuda, capi, orc, sigma):
    """viterbi::Viterbi27 (viterbi27.cpp: the decoder of the Meteor LRPT / Inmarsat plugin modules = CCDecoder on 2 F soft symbols with an
    erasure tail + MSB-first repack + re-encode BER x 4) as sdhip_op_viterbi27: six chained calls, clean / noisy / hopeless input with
    erased symbols in it -- decoded bytes and the per-call ber() bit-identical to the reference's."""
    import ctypes as C
    from oracle import pyref
    if not pyref.ref_available():
        pytest.skip("needs the compiled reference (viterbi27.cpp)")
    F, nf = 8192, 6
    rng = np.random.default_rng(5)
    tx = synth.conv_encode(rng.integers(0, 2, nf * F, dtype=np.uint8))
    soft = np.clip(np.rint((tx.astype(float) * 2 - 1) * 60 + rng.standard_normal(len(tx)) * sigma), -127, 127).astype(np.int8)
    soft[5] = 0
    soft[100:140] = 0
    want, wber = pyref.ref().viterbi27(F, soft, 1024)
    d_soft = torch_cuda.from_numpy(soft).cuda()
    d_out = torch_cuda.zeros((nf, F // 8), dtype=torch_cuda.uint8, device="cuda")
    ber = np.zeros(nf, dtype=np.float32)
    rc = capi.lib().sdhip_op_viterbi27(0, F, 1024, C.c_void_p(d_soft.data_ptr()), nf, C.c_void_p(d_out.data_ptr()), ber.ctypes.data_as(C.c_void_p))
    assert rc == 0, capi.lib().sdhip_last_error()
    assert np.array_equal(d_out.cpu().numpy(), want) and np.array_equal(ber, wber)


# ---------------------------------------------------------------- the RS tail over its whole argument space
# rs_type x I x basis x fill_bytes of k_rs / k_rs_screen / k_rs_screen4 (sdhip_op_rs_decode), then the module tail (k_rs_overrun, the
# filter trio) on the configurations of the reference's shipped pipelines.
_NROOTS = {"rs223": 32, "rs239": 16}
_RS_FRAMES = {}


def _rs_unit_frames(rs, I, dualbasis, fill, extra=0):
    """Frames of sdhip_op_rs_decode's matrix: 4 + (255 - max(fill, 0)) * I + extra bytes each (a code shortened by `fill` zero symbols in
    front of every codeword, `extra` random bytes behind the codeblock). With t = nroots / 2, codeword (f, b) carries (f + 3 b) mod (t + 4)
    byte errors at distinct positions, so every count from 0 to t + 3 occurs in every column: in the first (t + 4) frames in the message
    only (the decoder's count is then the number injected, up to t), in the next (t + 4) with the first message byte and the last parity
    byte among them, in the last (t + 4) in the parity only. Cached: the stride cases share the codewords of the matrix."""
    key = (rs, I, dualbasis, fill, extra)
    if key in _RS_FRAMES:
        return _RS_FRAMES[key]
    nroots = _NROOTS[rs]
    t, k, fb = nroots // 2, 255 - nroots, max(fill, 0)
    nfr = 3 * (t + 4)
    while nfr * I <= 64:  # more than one block of k_rs (64 codewords) for I = 1 too
        nfr += t + 4
    rng = np.random.default_rng(1000 * I + 10 * nroots + 2 * (fill + 1) + dualbasis)
    payload = rng.integers(0, 256, size=(nfr, I, k), dtype=np.uint8)
    payload[:, :, :fb] = synth._TO_DUAL[0] if dualbasis else 0
    full = synth.make_cadus(nfr, seed=0, rs_i=I, nroots=nroots, dualbasis=bool(dualbasis), derand=False, payload=payload)
    frames = np.concatenate([full[:, :4], full[:, 4 + fb * I:], rng.integers(0, 256, size=(nfr, extra), dtype=np.uint8)], axis=1)
    L = 255 - fb  # transmitted bytes of a codeword
    assert frames.shape[1] == 4 + L * I + extra
    for f in range(nfr):
        for b in range(I):
            n = (f + 3 * b) % (t + 4)
            if n == 0:
                continue
            cyc = (f // (t + 4)) % 3
            if cyc == 0:
                pos = rng.choice(L - nroots, size=n, replace=False)
            elif cyc == 1:
                pos = np.concatenate([[0, L - 1][:n], 1 + rng.choice(L - 2, size=max(n - 2, 0), replace=False)])
            else:
                pos = L - 1 - rng.choice(nroots, size=n, replace=False)
                if L - 1 not in pos:
                    pos[0] = L - 1
            assert len(set(int(p) for p in pos)) == n
            frames[f, 4 + pos.astype(np.int64) * I + b] ^= rng.integers(1, 256, size=n, dtype=np.uint8)
    _RS_FRAMES[key] = frames
    return frames


def _op_rs(torch, capi, frames, I, rs, dualbasis, fill):
    nfr, stride = frames.shape
    d = _dev(torch, frames.copy())  # (the cached frames stay as they are)
    d_err = torch.zeros(nfr * I, dtype=torch.int32, device="cuda")
    rc = capi.lib().sdhip_op_rs_decode(0, C.c_void_p(d.data_ptr() + 4), nfr, stride, int(dualbasis), I, capi.RS239 if rs == "rs239" else capi.RS223, fill,
                                       C.c_void_p(d_err.data_ptr()))
    assert rc == 0, capi.last_error()
    return d.cpu().numpy(), d_err.cpu().numpy().reshape(nfr, I)


@pytest.mark.parametrize("fill", [-1, 0, 3, 7, 16])
@pytest.mark.parametrize("dualbasis", [0, 1])
@pytest.mark.parametrize("I", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("rs", ["rs223", "rs239"])
def test_rs_decode_matrix(torch_cuda, capi, orc, rs, I, dualbasis, fill):
    """sdhip_op_rs_decode == ReedSolomon::decode_interlaved over RS(255,223) / RS(255,239), I = 1..8, both bases and shortened codes
    (rs_fill_bytes > 0), bit for bit in the data and in the nframes x I error counts. 3 (t + 4) frames (more for I = 1): partial last blocks
    of k_rs_screen (8 codewords), of k_rs_screen4 (8 frames) and of k_rs (64 codewords, more than one block)."""
    t = _NROOTS[rs] // 2
    frames = _rs_unit_frames(rs, I, dualbasis, fill)
    assert frames.shape[1] == 4 + (255 - max(fill, 0)) * I and len(frames) * I > 64
    want, ewant = orc.rs_decode(frames, I=I, dualbasis=bool(dualbasis), rs239=rs == "rs239", fill_bytes=fill)
    # the input does what it is meant to, by the oracle's answer alone: a failure, a correction of exactly t errors, a clean codeword
    assert (ewant == -1).any() and (ewant == t).any() and (ewant == 0).any()
    assert not np.array_equal(want, frames)
    got, egot = _op_rs(torch_cuda, capi, frames, I, rs, dualbasis, fill)
    assert np.array_equal(egot, ewant)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("rs", ["rs223", "rs239"])
def test_rs_decode_i4_through_the_generic_screen(torch_cuda, capi, orc, rs):
    """I = 4 with a frame stride that is no multiple of 4 (1026: two bytes behind the codeblock): launch_rs_only takes k_rs_screen instead of
    the packed k_rs_screen4, and the result is the stride-1024 result on the same codewords (and the oracle's)."""
    frames = _rs_unit_frames(rs, 4, 1, 0)
    wide = np.concatenate([frames, np.random.default_rng(3).integers(0, 256, size=(len(frames), 2), dtype=np.uint8)], axis=1)
    assert frames.shape[1] == 1024 and wide.shape[1] == 1026
    want, ewant = orc.rs_decode(frames, I=4, dualbasis=True, rs239=rs == "rs239", fill_bytes=0)
    got4, egot4 = _op_rs(torch_cuda, capi, frames, 4, rs, 1, 0)
    got, egot = _op_rs(torch_cuda, capi, wide, 4, rs, 1, 0)
    assert np.array_equal(egot4, ewant) and np.array_equal(got4, want)
    assert np.array_equal(egot, egot4) and np.array_equal(got[:, :1024], got4) and np.array_equal(got[:, 1024:], wide[:, 1024:])
    assert (ewant == -1).any() and (ewant > 0).any()


@pytest.mark.parametrize("I", [1, 4, 5, 8])
@pytest.mark.parametrize("rs", ["rs223", "rs239"])
def test_rs_decode_frame_longer_than_the_codeblock(torch_cuda, capi, orc, rs, I):
    """rs_fill_bytes = -1 with six random bytes behind the codeblock (stride 4 + 255 I + 6): the reference's 256-byte interleave leaves the
    first corrected message byte of codeword b (conventional basis) at offset 4 + 255 I + b of the frame after every successful decode;
    the op follows it wherever that offset lies inside the frame. All bytes of every frame are compared."""
    frames = _rs_unit_frames(rs, I, 1, -1, extra=6)
    assert frames.shape[1] == 4 + 255 * I + 6
    want, ewant = orc.rs_decode(frames, I=I, dualbasis=True, rs239=rs == "rs239", fill_bytes=-1)
    assert (ewant == -1).any() and (ewant >= 0).any()
    assert not np.array_equal(want[:, 4 + 255 * I:], frames[:, 4 + 255 * I:])  # the overrun is visible in the oracle's answer
    got, egot = _op_rs(torch_cuda, capi, frames, I, rs, 1, -1)
    assert np.array_equal(egot, ewant)
    assert np.array_equal(got, want)


def _gf_solve3(A, y):
    """x with sum_i A[j][i] x_i = y_j over GF(256) (3 x 3, Gauss-Jordan)."""
    inv = lambda a: int(synth._EXP[(255 - synth._LOG[a]) % 255])
    mul = lambda a, b: int(synth.gf_mul(a, b))
    M = [[int(v) for v in r] + [int(v)] for r, v in zip(A, y)]
    for c in range(3):
        p = next(r for r in range(c, 3) if M[r][c])
        M[c], M[p] = M[p], M[c]
        M[c] = [mul(v, inv(M[c][c])) for v in M[c]]
        for r in range(3):
            if r != c and M[r][c]:
                M[r] = [a ^ mul(M[r][c], b) for a, b in zip(M[r], M[c])]
    return [M[j][3] for j in range(3)]


def _force_last_parity(conv, nroots, target):
    """conv [n, k] messages (conventional basis): their first three bytes chosen so that the last three parity bytes are `target`."""
    g = synth.rs_generator(nroots, 112 if nroots == 32 else 120, 11)[1:]
    k = conv.shape[1]
    unit = synth._rs_lfsr(np.eye(k, dtype=np.uint8)[:3], g)[:, -3:]  # [message position, parity byte]
    conv = conv.copy()
    conv[:, :3] = 0
    p0 = synth._rs_lfsr(conv, g)[:, -3:]
    for n in range(len(conv)):
        conv[n, :3] = _gf_solve3(unit.T, p0[n] ^ np.asarray(target, dtype=np.uint8))
    assert np.array_equal(synth._rs_lfsr(conv, g)[:, -3:], np.broadcast_to(np.asarray(target, dtype=np.uint8), (len(conv), 3)))
    return conv


# name: (decoder, constellation, nrzm, cadu_size, rs_i, rs type, rs_fill_bytes, rs_dualbasis, junk prefix in soft bytes); modelled on the
# reference's shipped pipelines (the name), see DESIGN.md (parity contract: the RS tail)
_TAIL_CASES = {
    "integral": ("concat", "bpsk_90", 1, 8192, 4, "rs239", -1, 1, 3000),
    "queqiao": ("concat", "bpsk_90", 1, 2048, 1, "rs223", 3, 1, 3000),
    "slim": ("concat", "bpsk", 1, 2048, 1, "rs223", -1, 1, 5000),
    "slim_first_frame_alone": ("concat", "bpsk", 1, 2048, 1, "rs223", -1, 1, 1000),  # the first frame ends in the second half of its call
    "tianwen": ("concat", "bpsk_90", 1, 2048, 1, "rs223", -1, 0, 1000),
    "qpsk_i5_rs223": ("concat", "qpsk", 1, 10232, 5, "rs223", -1, 1, 3000),
    "qpsk_i5_rs239": ("concat", "qpsk", 1, 10232, 5, "rs239", -1, 1, 3000),
    "qpsk_i5_fill3": ("concat", "qpsk", 1, 10112, 5, "rs239", 3, 1, 3000),
    "qpsk_i8": ("concat", "qpsk", 1, 16352, 8, "rs223", -1, 1, 3000),
    "long_frame_2080": ("concat", "bpsk", 1, 2080, 1, "rs223", -1, 1, 3000),  # the frame is 4 bytes longer than the codeblock
    "aim": ("simple", "bpsk", 1, 9952, 5, "rs223", 7, 1, 3000),
    "simple_qpsk_fill16": ("simple", "qpsk", 0, 9592, 5, "rs223", 16, 1, 3000),
    "oceansat": ("simple", "qpsk", 0, 16352, 8, "rs239", -1, 1, 3000),
    "simple_bpsk_fill9": ("simple", "bpsk", 0, 2000, 1, "rs223", 9, 1, 3000),
    "simple_bpsk_2048": ("simple", "bpsk", 0, 2048, 1, "rs223", -1, 1, 3000),
}
_TAIL_CACHE = {}
# streams whose first deframed frame is the only one of its deframer call (4096 bits, two frames as a rule: the junk prefix puts its end
# into the second half of a call) AND carries t message errors: behind it the reference reads the zeros its frame buffer starts with
_FIRST_FRAME_ALONE = ("slim_first_frame_alone", "tianwen")


def _tail_case(name):
    """(soft stream, transmitted frames before randomising and errors) of one _TAIL_CASES row: a junk prefix, CADUs with 0, a few, t, t + 3 and
    40 byte errors, all in ONE codeword column of a frame (spread over five or eight columns they never reach a failure), a noise tail.
    Frames shorter than their codeblock (2048 bits, I = 1, fill -1) are cut, and their codewords are chosen so that the three parity bytes
    cut off ARE 1A CF FC: the decoder then sees no error there when the reference reads a sync marker behind the frame and three when it
    reads zeros, which decides the frames with t - 2 .. t errors."""
    if name in _TAIL_CACHE:
        return _TAIL_CACHE[name]
    dec, const, nrzm, cadu_size, I, rs, fill, dual, prefix = _TAIL_CASES[name]
    nroots = _NROOTS[rs]
    t, k, fb, nb = nroots // 2, 255 - nroots, max(fill, 0), cadu_size // 8
    nfr = 6 if cadu_size > 8192 else 30  # (the host twin of the Viterbi decoder takes a second per long frame)
    rng = np.random.default_rng(cadu_size + 7 * I + nroots + prefix)
    payload = rng.integers(0, 256, size=(nfr, I, k), dtype=np.uint8)
    payload[:, :, :fb] = synth._TO_DUAL[0] if dual else 0
    short = nb < 4 + (255 - fb) * I
    if short:
        asm3 = np.array([0x1A, 0xCF, 0xFC], dtype=np.uint8)
        conv = _force_last_parity((synth._FROM_DUAL[payload] if dual else payload).reshape(-1, k), nroots, synth._FROM_DUAL[asm3] if dual else asm3)
        payload = (synth._TO_DUAL[conv] if dual else conv).reshape(nfr, I, k)
    full = synth.make_cadus(nfr, seed=0, rs_i=I, nroots=nroots, dualbasis=bool(dual), derand=False, payload=payload)
    body = full[:, 4 + fb * I:]
    if short:
        assert np.array_equal(body[0, nb - 4:], asm3)
    if body.shape[1] < nb - 4:
        body = np.concatenate([body, rng.integers(0, 256, size=(nfr, nb - 4 - body.shape[1]), dtype=np.uint8)], axis=1)
    body = body[:, :nb - 4]
    plain = np.concatenate([full[:, :4], body], axis=1)
    tx = plain.copy()
    counts = [0, 3, t, t + 3, 40, 0, t - 1, t - 2, 1, t]
    if name in _FIRST_FRAME_ALONE:  # the first frame decodes only if a sync marker is read behind it (_assert_first_frame_reads_zeros)
        counts = [t] + counts
    for f in range(nfr):
        b = f % I
        npos = min(255 - fb, (nb - 4 - b + I - 1) // I)  # the codeword's bytes inside the frame
        pos = rng.choice(min(npos, k - fb), size=counts[f % len(counts)], replace=False)  # (in the message: the count is what RS reports)
        tx[f, 4 + pos * I + b] ^= rng.integers(1, 256, size=len(pos), dtype=np.uint8)
    tx[:, 4:] ^= np.resize(synth.ccsds_pn_table(), nb - 4)[None, :]
    junk = rng.integers(-90, 90, prefix).astype(np.int8)
    if dec == "concat":
        sp = synth.SynthSpec(constellation="qpsk" if const == "qpsk" else "bpsk", nrzm=bool(nrzm), seed=9)
        soft = synth.soft_from_symbols(synth.frames_to_symbols(tx, sp), sp, sigma=15.0, seed=4)
        if const == "bpsk_90":  # the module swaps I and Q and decodes at PHASE_90: a bpsk stream with every odd soft byte negated
            soft = soft.copy()
            soft[1::2] = -soft[1::2]
        B = max(cadu_size, 8192)
        soft = np.concatenate([junk, soft, rng.integers(-127, 128, B + 2048).astype(np.int8)])
        soft = soft[: len(soft) // B * B]
    else:
        soft = util.simple_soft(tx, constellation=const, nrzm=bool(nrzm), sigma=15.0, seed=6)
        soft = np.concatenate([junk, soft, rng.integers(-90, 90, 2 * cadu_size).astype(np.int8)])
    _TAIL_CACHE[name] = (soft, plain)
    return _TAIL_CACHE[name]


def _tail_kw(name, usecheck):
    dec, const, nrzm, cadu_size, I, rs, fill, dual, _ = _TAIL_CASES[name]
    return dict(nrzm=nrzm, cadu_size=cadu_size, rs_i=I, rs_fill_bytes=fill, rs_dualbasis=dual, rs_usecheck=usecheck)


def _tail_ocfg(name, usecheck):
    dec, const, rs = _TAIL_CASES[name][0], _TAIL_CASES[name][1], _TAIL_CASES[name][5]
    return pyref.fec_cfg(decoder=2 if dec == "simple" else 0, constellation=getattr(pyref, const.upper()), rs_type=pyref.RS239 if rs == "rs239" else pyref.RS223,
                         **_tail_kw(name, usecheck))


def _tail_cfg(capi, name, usecheck):
    dec, const, rs = _TAIL_CASES[name][0], _TAIL_CASES[name][1], _TAIL_CASES[name][5]
    return capi.fec_cfg(decoder=capi.DEC_SIMPLE_PSK if dec == "simple" else capi.DEC_CONV_CONCAT, constellation=const,
                        rs_type=capi.RS239 if rs == "rs239" else capi.RS223, **_tail_kw(name, usecheck))


def _tail_want(orc, name, usecheck):
    key = (name, usecheck, orc.path)
    if key not in _TAIL_CACHE:
        soft, plain = _tail_case(name)
        oc = _tail_ocfg(name, usecheck)
        _TAIL_CACHE[key] = orc.simple_decode(oc, soft) if _TAIL_CASES[name][0] == "simple" else orc.concat_decode(oc, soft)
    return _TAIL_CACHE[key]


def _assert_tail_input(name, want, plain, usecheck):
    """By the oracle's answer alone: a frame with a failed codeword, a corrected frame, a frame that left as it was transmitted. (In a frame
    longer than its codeblock every successful decode rewrites the bytes at 4 + 255 I + b of the frame itself: there the transmitted frame
    is looked for in the other bytes, and the rewritten ones must differ from it somewhere.)"""
    _, _, _, cadu_size, I, _, fill, _, _ = _TAIL_CASES[name]
    fe = want["frm_err"]
    assert len(fe) == want["n_deframed"] and len(fe) >= (5 if cadu_size > 8192 else 20)
    assert (fe == -1).any(1).any(), "no frame with an uncorrectable codeword"
    assert ((fe >= 0).all(1) & (fe > 0).any(1)).any(), "no corrected frame"
    cols = np.ones(plain.shape[1], dtype=bool)
    if fill == -1:
        cols[4 + 255 * I: 4 + 256 * I] = False
    hits = [c for c in want["cadu"] if (plain[:, cols] == c[cols]).all(1).any()]
    assert hits, "no frame equal to a transmitted one"
    if not cols.all():
        assert any(not (plain == c).all(1).any() for c in hits), "the overrun into the frame's own tail is not visible"
    if usecheck:
        assert len(want["cadu"]) == int((fe != -1).all(1).sum())
    else:
        assert len(want["cadu"]) == len(fe)


def _assert_first_frame_reads_zeros(orc, name):
    """By the oracle alone: the first deframed frame of a _FIRST_FRAME_ALONE stream fails (t message errors and, behind the frame, three zeros
    where its parity bytes 1A CF FC were cut off), and the very same frame decodes with t errors once a sync marker stands behind it. So a
    decoder that reads a marker there -- a successor's, or one it wrongly believes an earlier call left -- gives another answer."""
    _, _, _, cadu_size, I, rs, fill, dual, _ = _TAIL_CASES[name]
    assert (cadu_size, I, fill) == (2048, 1, -1)
    t = _NROOTS[rs] // 2
    w = _tail_want(orc, name, 0)  # rs_usecheck off: every deframed frame is there, a failed one as RS saw it
    assert w["frm_err"][0][0] == -1 and w["frm_err"][1][0] >= 0
    seen = w["cadu"][0]
    for behind, result in (([0x1A, 0xCF, 0xFC], t), ([0, 0, 0], -1)):
        frame = np.concatenate([seen, np.array(behind, dtype=np.uint8)])[None, :]
        _, e = orc.rs_decode(frame, I=1, dualbasis=bool(dual), rs239=rs == "rs239", fill_bytes=-1)
        assert e[0][0] == result, (behind, e)


@pytest.mark.parametrize("usecheck", [0, 1])
@pytest.mark.parametrize("name", list(_TAIL_CASES))
def test_rs_tail_of_the_shipped_pipelines(torch_cuda, capi, orc, name, usecheck):
    """The frame tail (k_extract, k_rs_screen, k_rs, k_rs_overrun, k_derand, the k_rs_keep / filter / slots trio) through FecDecoder ==
    the reference's module loop on RS(255,239), I = 1, 5 and 8, shortened codes, bpsk_90 and frames shorter and longer than their codeblock:
    CADUs, frames deframed, the last frame's error counts and, for the concatenated decoder, the per-block BER and state."""
    dec, I = _TAIL_CASES[name][0], _TAIL_CASES[name][4]
    soft, plain = _tail_case(name)
    want = _tail_want(orc, name, usecheck)
    _assert_tail_input(name, want, plain, usecheck)
    if name in _FIRST_FRAME_ALONE:
        _assert_first_frame_reads_zeros(orc, name)
    cfg = _tail_cfg(capi, name, usecheck)
    got, ber, state, st = _run_dev(torch_cuda, capi, cfg, soft)
    assert st.frames_deframed == want["n_deframed"]
    assert list(st.rs_errors[:I]) == [int(e) for e in want["frm_err"][-1]]
    if dec == "concat":
        assert np.array_equal(state, want["state"])
        assert np.array_equal(ber.view(np.uint32), want["ber"].view(np.uint32))
    assert got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"])


@pytest.mark.parametrize("name", ["slim", "slim_first_frame_alone", "tianwen", "simple_bpsk_2048"])
def test_rs_tail_short_frames_in_ragged_calls(torch_cuda, capi, orc, name):
    """Frames three bytes shorter than their codeblock, pushed in ragged calls: the last frame of a batch has its successor only in the next
    call, and what RS reads behind it is what the reference's frame buffer holds there (zeros until that slot was written once, a sync
    marker afterwards), never what the device buffer happens to hold."""
    soft, plain = _tail_case(name)
    want = _tail_want(orc, name, 1)
    _assert_tail_input(name, want, plain, 1)
    if name in _FIRST_FRAME_ALONE:
        _assert_first_frame_reads_zeros(orc, name)
    cfg = _tail_cfg(capi, name, 1)
    n = len(soft)
    bounds = [0, 1000, 1000, 8192 * 3 + 17, 8192 * 4, 8192 * 7 + 5, 8192 * 8, n]
    got, _, _, st = _run_dev(torch_cuda, capi, cfg, soft, chunks=bounds)
    assert st.frames_deframed == want["n_deframed"]
    assert got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"])


def test_rs_overrun_into_the_next_frames_data_is_refused(torch_cuda, capi):
    """rs_fill_bytes = -1 writes the first corrected byte of codeword b at offset 4 + 255 I + b from the frame's start. Where that is byte 4
    or later of a successor from the same deframer call, the reference decodes the successor with that byte changed, which the parallel
    tail does not reproduce: the configuration is refused when the handle is created. The refusal is conditional on such a successor being
    possible, i.e. on a CADU shorter than the bits of one deframer call (max(cadu_size, 8192) / 2 at rate 1/2): longer CADUs with the same
    target (every rs_i >= 5 pipeline) have no same-call successor, nothing is written, and they are accepted."""
    def create(**kw):
        capi.FecDecoder(capi.fec_cfg(constellation="bpsk", nrzm=1, rs_type=capi.RS223, **kw)).close()
    for kw in (dict(cadu_size=2040, rs_i=1, rs_fill_bytes=-1),   # 255 bytes: codeword 0 -> byte 4 of the successor
               dict(cadu_size=4088, rs_i=2, rs_fill_bytes=-1)):  # 511 bytes, 4088 < 4096 bits a call: codeword 1 -> byte 4
        with pytest.raises(capi.SdhipError, match="overrun"):
            create(**kw)
    create(cadu_size=4096, rs_i=2, rs_fill_bytes=-1)   # 512 bytes: codeword 1 -> byte 3, the marker's last
    create(cadu_size=8160, rs_i=4, rs_fill_bytes=-1)   # 1020 bytes: codeword 3 -> byte 7, but one frame a call at most
    create(cadu_size=10232, rs_i=5, rs_fill_bytes=-1)  # codeword 4 -> byte 4, one frame a call at most
    create(cadu_size=2040, rs_i=1, rs_fill_bytes=0)    # no 256th byte: nothing overruns
    with pytest.raises(capi.SdhipError, match="does not fit"):
        create(cadu_size=2000, rs_i=1, rs_fill_bytes=0)
    # a shortened code keeps at least one message byte: rs_fill_bytes < 255 - nroots, in the handle and in the op
    with pytest.raises(capi.SdhipError, match="rs_fill_bytes out of range"):
        create(cadu_size=8 * (4 + 32), rs_i=1, rs_fill_bytes=223)
    create(cadu_size=8 * (4 + 33), rs_i=1, rs_fill_bytes=222)
    d = torch_cuda.zeros(64, dtype=torch_cuda.uint8, device="cuda")
    d_err = torch_cuda.zeros(1, dtype=torch_cuda.int32, device="cuda")
    op = lambda rs, fill: capi.lib().sdhip_op_rs_decode(0, C.c_void_p(d.data_ptr() + 4), 1, 4 + 255 - fill, 1, 1, rs, fill, C.c_void_p(d_err.data_ptr()))
    assert op(capi.RS223, 223) != 0 and "out of range" in str(capi.last_error())
    assert op(capi.RS239, 239) != 0 and op(capi.RS223, -2) != 0
    assert op(capi.RS239, 238) == 0, capi.last_error()
