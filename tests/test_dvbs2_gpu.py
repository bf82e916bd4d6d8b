"""GPU parity tests of the DVB-S2 LDPC decoder (sdhip_ldpc_*, satdump_amd/csrc/dvbs2_ldpc.hip) against the reference's own BBFrameLDPC
compiled in place (oracle/_ref/libsdref_dvbs2*.so, oracle/ref_wrap_dvbs2.cpp). Integer work: the decoded soft bits and the trial counts
must be IDENTICAL -- converged or not, and in the 16-frames-per-call grouping of the reference's SSE4.1 build (one early exit per call)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import pyref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    # torch first: its bundled HIP runtime must be the one that initialises the device (loading libsdhip.so first and torch.cuda later
    # left torch with "No HIP GPUs are available" on the GPU box)
    import torch
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")
    from satdump_amd import capi as c
    c.lib()
    return c


def _ref(sse):
    if not pyref.Dvbs2Ref.available(sse):
        pytest.skip("oracle/_ref/libsdref_dvbs2*.so not built (needs /root/reference at build time)")
    return pyref.Dvbs2Ref(sse=sse)


def make_frames(ref, fs, rate_code, nframes, amp, sigma, seed):
    """LDPC code words of random data (tests/dvbs2_util.py: the accumulator encoder of the standard, from the same address tables),
    BPSK-mapped like the soft demapper's output (bit 1 -> negative), plus noise, clipped to int8."""
    from tests import dvbs2_util
    n, k = ref.dims(fs, rate_code)
    rng = np.random.default_rng(seed)
    bits = dvbs2_util.encode(fs, rate_code, rng.integers(0, 2, (nframes, k), dtype=np.uint8))
    assert bits.shape[1] == n
    soft = np.where(bits > 0, -1.0, 1.0) * amp + rng.standard_normal(bits.shape) * sigma
    return np.clip(np.rint(soft), -127, 127).astype(np.int8), bits, k


def run_case(capi, ref, fs, rate, nframes, amp, sigma, trials, seed=1):
    rc = capi.S2_RATES[rate]
    nframes = (nframes + ref.batch - 1) // ref.batch * ref.batch
    soft, bits, k = make_frames(ref, fs, rc, nframes, amp, sigma, seed)
    want, wt = ref.ldpc_decode(fs, rc, soft, trials)
    dec = capi.LdpcDecoder(framesize=fs, rate=rate, batch=ref.batch)
    got = soft.copy()
    gt = dec.decode(got, trials)
    assert np.array_equal(gt, wt), (gt.tolist(), wt.tolist())
    assert np.array_equal(got, want)
    return got, gt, bits, k, dec


NORMAL = ["1/4", "1/3", "2/5", "1/2", "3/5", "2/3", "3/4", "4/5", "5/6", "8/9", "9/10"]
SHORT = ["1/4", "1/3", "2/5", "1/2", "3/5", "2/3", "3/4", "4/5", "5/6", "8/9"]
# noise (for unit amplitude 20) at which each rate needs a handful of iterations
SIGMA = {"1/4": 26, "1/3": 23, "2/5": 21, "1/2": 18, "3/5": 15, "2/3": 13.5, "3/4": 12, "4/5": 11, "5/6": 10, "8/9": 8, "9/10": 7.5}


@pytest.mark.parametrize("fs,rate", [(0, r) for r in NORMAL] + [(1, r) for r in SHORT])
def test_every_code_bit_exact(capi, fs, rate):
    """All 21 tables of the standard (annex B normal, annex C short): clean frames (0 update passes), frames near the waterfall
    (some converge, some do not) and hopeless ones (-1) -- soft bits and trial counts identical to the reference's."""
    ref = _ref(False)
    got, gt, bits, k, dec = run_case(capi, ref, fs, rate, 3, 20, SIGMA[rate] * (1.0 if fs == 0 else 0.9), 12)
    assert dec.info.code_len == (64800 if fs == 0 else 16200) and dec.info.data_len == k
    run_case(capi, ref, fs, rate, 1, 60, 1.0, 5, seed=2)   # clean: converged before the first update
    run_case(capi, ref, fs, rate, 1, 5, 30.0, 3, seed=3)   # noise: never converges
    conv = gt >= 0
    if conv.any():
        assert np.array_equal((got[conv][:, :k] < 0).astype(np.uint8), bits[conv][:, :k]), "a converged frame does not carry the transmitted data"


@pytest.mark.parametrize("fs,rate", [(0, "2/3"), (0, "3/4"), (1, "1/2"), (1, "8/9")])
def test_sse_batches_share_one_early_exit(capi, fs, rate):
    """The reference's x86 build decodes 16 frames per call and stops when ALL of them have converged (layered_decoder.hh:160,
    algorithms.hh:264-271): frames that are done keep being updated. batch = 16 reproduces that bit for bit; mixed batches (a noisy
    frame among clean ones) are what distinguishes it from batch = 1."""
    ref = _ref(True)
    assert ref.batch == 16
    rc = capi.S2_RATES[rate]
    soft, bits, k = make_frames(ref, fs, rc, 32, 20, SIGMA[rate] * (1.0 if fs == 0 else 0.9), 5)
    clean, _, _ = make_frames(ref, fs, rc, 32, 60, 1.0, 5)
    soft[3:16] = clean[3:16]  # first batch: three noisy frames among clean ones
    want, wt = ref.ldpc_decode(fs, rc, soft, 15)
    dec = capi.LdpcDecoder(framesize=fs, rate=rate, batch=16)
    got = soft.copy()
    gt = dec.decode(got, 15)
    assert np.array_equal(gt, wt) and np.array_equal(got, want)
    one = capi.LdpcDecoder(framesize=fs, rate=rate, batch=1)
    solo = soft.copy()
    one.decode(solo, 15)
    if wt[0] > 0:
        assert not np.array_equal(solo[3:16], got[3:16]), "clean frames of a mixed batch should have been updated along with the noisy ones"


def rails_case(capi, fs, rate, sse):
    """Frames at amplitude 60, sigma 25, clipped to the WHOLE int8 range (make_frames stops at +-127): -128 among the inputs."""
    from tests import dvbs2_util
    ref = _ref(sse)
    rc = capi.S2_RATES[rate]
    n, k = ref.dims(fs, rc)
    nframes = 16 if sse else 3
    rng = np.random.default_rng(60 + fs)
    bits = dvbs2_util.encode(fs, rc, rng.integers(0, 2, (nframes, k), dtype=np.uint8))
    soft = np.clip(np.rint(np.where(bits > 0, -1.0, 1.0) * 60 + rng.standard_normal(bits.shape) * 25.0), -128, 127).astype(np.int8)
    assert ((soft == -128).sum(1) > 0).all() and ((soft == 127).sum(1) > 0).all()
    want, wt = ref.ldpc_decode(fs, rc, soft, 12)
    assert (wt >= 0).all() and np.array_equal((want[:, :k] < 0).astype(np.uint8), bits[:, :k])  # by the reference alone: the frames decode, to the data sent
    dec = capi.LdpcDecoder(framesize=fs, rate=rate, batch=ref.batch)
    got = soft.copy()
    gt = dec.decode(got, 12)
    assert np.array_equal(gt, wt), (gt.tolist(), wt.tolist())
    assert np.array_equal(got, want)


@pytest.mark.parametrize("sse", [False, True], ids=["generic_batch1", "sse_batch16"])
@pytest.mark.parametrize("fs,rate", [(0, "2/3"), (1, "1/2")])
def test_int8_rail_inputs(capi, fs, rate, sse):
    """-128 at the LDPC decoder's input (tests/test_soft_rails_gpu.py has the other decoders): soft bits and trial counts identical to the reference's, batch = 1
    against its generic build and batch = 16 against its SSE4.1 build -- each mode is held to the build it mirrors, whatever the two builds make of -128
    between themselves. The reference's own demapper cannot emit -128: constellation_t::clamp (constellation.cpp:289-298, behind demod_soft_calc's LLRs, which
    demod_soft_lut's table holds; dvbs2_bb_to_soft.cpp:62) halves a finite value until it lies in [-127, 127] and truncates towards zero, and a non-finite one is
    converted as it is (not defined by the language; 0 on x86). So -128 reaches BBFrameLDPC only from another producer's soft frames, which the entry accepts."""
    rails_case(capi, fs, rate, sse)


def test_device_entry_and_many_frames(capi):
    """sdhip_ldpc_decode_dev on frames resident in HBM, a few hundred frames (more workgroups than CUs), normal 2/3 (BASELINE configs[4]'s
    MODCOD 13): identical to the reference on all of them, and (size-independent property) the converged frames carry their data."""
    import torch
    ref = _ref(False)
    rc = capi.S2_RATES["2/3"]
    n, k = ref.dims(0, rc)
    nf = 600
    soft, bits, _ = make_frames(ref, 0, rc, nf, 20, 13.0, 7)
    d = torch.from_numpy(soft).cuda()
    d_tr = torch.zeros(nf, dtype=torch.int32, device="cuda")
    dec = capi.LdpcDecoder(framesize=0, rate="2/3", batch=1)
    dec.decode_dev(d.data_ptr(), nf, 20, d_tr.data_ptr())
    got, tr = d.cpu().numpy(), d_tr.cpu().numpy()
    want, wt = ref.ldpc_decode(0, rc, soft, 20)  # ~10 s of one host core
    assert np.array_equal(tr, wt) and np.array_equal(got, want)
    conv = tr >= 0
    assert conv.mean() > 0.9
    # (a frame can "converge" onto a neighbouring code word -- here one of 600 ends two data bits off, in the reference too: that is what
    # the BCH outer code behind the decoder is for)
    right = [np.array_equal(got[i, :k] < 0, bits[i, :k] > 0) for i in np.flatnonzero(conv)]
    assert np.mean(right) > 0.99


def bch_case(capi, ref, fs, rate, errs, seed=3):
    """Random BCH code words (the reference's encoder) with errs[i] bit errors in frame i, through both decoders."""
    rc = capi.S2_RATES[rate]
    dec = capi.BchDecoder(framesize=fs, rate=rate)
    assert dec.kbch == ref.bch_kbch(fs, rc)
    rng = np.random.default_rng(seed)
    fr = np.zeros((len(errs), dec.nbch // 8), dtype=np.uint8)
    fr[:, :dec.kbch // 8] = rng.integers(0, 256, (len(errs), dec.kbch // 8), dtype=np.uint8)
    cw = ref.bch_encode(fs, rc, fr)
    rx = cw.copy()
    for i, e in enumerate(errs):
        for p in rng.choice(dec.nbch, e, replace=False):
            rx[i, p // 8] ^= 1 << (7 - p % 8)
    want, wc = ref.bch_decode(fs, rc, rx)
    got = rx.copy()
    gc = dec.decode(got)
    assert np.array_equal(gc, wc), (gc.tolist(), wc.tolist())
    assert np.array_equal(got, want)
    return cw, got, gc, dec


@pytest.mark.parametrize("fs,rate", [(0, r) for r in NORMAL] + [(1, r) for r in SHORT])
def test_bch_every_code_bit_exact(capi, fs, rate):
    """BBFrameBCH::decode for every frame size / rate (t = 12 / 10 / 8 over GF(2^16), t = 12 over GF(2^14)): clean frames, 1 .. t errors
    (degree 1 and 2 locators take the closed-form finders, the rest the Chien search), and t + 1 .. many errors, where the decoder gives
    up (-1, frame untouched) or miscorrects -- corrected bytes and return values identical to the reference's."""
    ref = _ref(False)
    errs = [0, 1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 13, 16, 30, 200]
    cw, got, gc, dec = bch_case(capi, ref, fs, rate, errs)
    t = {0: {"2/3": 10, "5/6": 10, "8/9": 8, "9/10": 8}.get(rate, 12), 1: 12}[fs]
    for i, e in enumerate(errs):
        if e <= t:
            assert gc[i] == e and np.array_equal(got[i], cw[i])


def test_ldpc_pack_bch_chain_on_device(capi):
    """The FEC tail of DVBS2DemodModule::process_s2 on frames resident in HBM: LDPC decode -> hard-decision repack -> BCH decode
    -> BB descrambler (module_dvbs2_demod.cpp:254-273), against the same four steps of the reference; normal 2/3 (MODCOD 13 of BASELINE configs[4])."""
    import torch
    from tests import dvbs2_util
    ref = _ref(False)
    fs, rate, rc = 0, "2/3", 5
    n, k = ref.dims(fs, rc)
    bch = capi.BchDecoder(framesize=fs, rate=rate)
    assert bch.nbch == k
    nf = 24
    rng = np.random.default_rng(11)
    bb = np.zeros((nf, k // 8), dtype=np.uint8)
    bb[:, :bch.kbch // 8] = rng.integers(0, 256, (nf, bch.kbch // 8), dtype=np.uint8)
    bb = ref.bch_encode(fs, rc, bb)                                     # BBFRAME + BCH parity = the LDPC data bits
    cw = dvbs2_util.encode(fs, rc, np.unpackbits(bb, axis=1))
    soft = np.clip(np.rint(np.where(cw > 0, -1.0, 1.0) * 20 + rng.standard_normal(cw.shape) * 14.0), -127, 127).astype(np.int8)
    # reference chain
    rsoft, rtr = ref.ldpc_decode(fs, rc, soft, 20)
    rpack = np.packbits((rsoft[:, :k] < 0).astype(np.uint8), axis=1)
    rout, rcorr = ref.bch_decode(fs, rc, rpack)
    rdes = ref.bb_descramble(fs, rc, rout)
    # device chain
    d_soft = torch.from_numpy(soft.copy()).cuda()
    d_tr = torch.zeros(nf, dtype=torch.int32, device="cuda")
    d_pack = torch.zeros((nf, k // 8), dtype=torch.uint8, device="cuda")
    d_corr = torch.zeros(nf, dtype=torch.int32, device="cuda")
    ldpc = capi.LdpcDecoder(framesize=fs, rate=rate, batch=1)
    ldpc.decode_dev(d_soft.data_ptr(), nf, 20, d_tr.data_ptr())
    bch.pack_dev(d_soft.data_ptr(), n, nf, d_pack.data_ptr(), k // 8)
    bch.decode_dev(d_pack.data_ptr(), nf, k // 8, d_corr.data_ptr())
    assert np.array_equal(d_tr.cpu().numpy(), rtr)
    assert np.array_equal(d_pack.cpu().numpy(), rout) and np.array_equal(d_corr.cpu().numpy(), rcorr)
    bch.descramble_dev(d_pack.data_ptr(), nf, k // 8)  # BBFrameDescrambler::work, the last step of process_s2 (module_dvbs2_demod.cpp:273)
    assert np.array_equal(d_pack.cpu().numpy(), rdes)
    good = rcorr >= 0
    assert good.mean() > 0.5 and np.array_equal(rout[good][:, :bch.kbch // 8], bb[good][:, :bch.kbch // 8])


@pytest.mark.parametrize("const,fs,rate", [(0, 0, 5), (1, 0, 5), (1, 0, 4), (1, 1, 4), (2, 0, 6), (2, 1, 6), (3, 0, 7), (3, 1, 7)])
def test_s2_deinterleaver(capi, const, fs, rate):
    """dvbs2::S2Deinterleaver::deinterleave (the step between the soft demapper and the LDPC decoder, dvbs2_bb_to_soft.cpp:63): QPSK pair
    swap, 8PSK / 16APSK / 32APSK column de-interleaving, 8PSK rate 3/5 with its reversed column order -- identical bytes."""
    import ctypes as C
    import torch
    ref = _ref(False)
    n = 64800 if fs == 0 else 16200
    x = np.random.default_rng(const + rate).integers(-128, 128, (5, n), dtype=np.int8)
    want = ref.s2_deinterleave(const, fs, rate, x)
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.zeros_like(d_in)
    rc = capi.lib().sdhip_s2_deinterleave_dev(0, const, fs, rate, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), 5)
    assert rc == 0 and np.array_equal(d_out.cpu().numpy(), want)


BB2SOFT = [(6, 0, 0), (4, 1, 0), (13, 0, 0), (12, 1, 0), (20, 0, 0), (23, 1, 0), (6, 0, 1), (13, 1, 1), (18, 0, 1)]


def check_bb_to_soft(capi, to_dev, from_dev, zeros_dev, modcod, short, pilots, nframes=4):
    """sdhip_s2_bb_to_soft_dev == dvbs2::S2BBToSoft::work frame by frame (the reference block driven through its own dsp::stream input and
    output, oracle/ref_wrap_dvbs2_demap.cpp): decoded PLS index, PL descrambling, table demapping, pilots branch, de-interleaver -- identical
    soft bits. The demapper table is the reference's own (constellation_t::make_lut(256)), handed over as the binding's caller would."""
    import ctypes as C
    from tests import dvbs2_util
    if not pyref.S2FrontRef.available():
        pytest.skip("oracle/_ref/libsdref_dvbs2.so without the front-end entries (rebuild with the reference tree)")
    ref = pyref.S2FrontRef()
    c = ref.cfg(modcod, short, pilots)
    pls_index = (modcod << 2) | (short << 1) | pilots
    fr = dvbs2_util.plframes(c["slots"], pls_index, nframes, seed=modcod + 7 * short + pilots)
    want, wpls = ref.bb_to_soft(modcod, short, pilots, fr)
    assert np.all(wpls == pls_index)  # three inverted header symbols are inside the code's distance
    lut = ref.lut(modcod, short)
    d_fr = to_dev(fr.view(np.float32))
    nsoft = c["slots"] * 90 * c["bits"]
    d_soft = zeros_dev(nframes * nsoft, np.int8)
    d_pls = zeros_dev(nframes, np.int32)
    rc = capi.lib().sdhip_s2_bb_to_soft_dev(0, modcod, short, pilots, C.c_void_p(d_fr[1]), fr.shape[1], nframes, lut.ctypes.data_as(C.c_void_p), 256,
                                            C.c_void_p(d_soft[1]), C.c_void_p(d_pls[1]))
    assert rc == nsoft, capi.last_error()
    got = from_dev(d_soft).reshape(nframes, nsoft)
    assert np.array_equal(from_dev(d_pls), wpls)
    assert np.array_equal(got, want)
    assert nsoft == (16200 if short else 64800) and np.count_nonzero(got) > 0.9 * got.size * (0.9 if pilots else 1.0)


@pytest.mark.parametrize("modcod,short,pilots", BB2SOFT)
def test_bb_to_soft(capi, modcod, short, pilots):
    import torch

    def to_dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return (t, t.data_ptr())

    def zeros_dev(n, dt):
        t = torch.zeros(n, dtype={np.int8: torch.int8, np.int32: torch.int32}[dt], device="cuda")
        return (t, t.data_ptr())

    check_bb_to_soft(capi, to_dev, lambda d: d[0].cpu().numpy(), zeros_dev, modcod, short, pilots)


PLSYNC = [(90, 0, "slips"), (60, 1, "slips"), (45, 0, "locked"), (90, 0, "noise"), (360, 0, "slips")]


def check_pl_sync(capi, to_dev, from_dev, zeros_dev, slots, pilots, kind):
    """sdhip_s2_pl_sync_dev == dvbs2::S2PLSyncBlock::work2 frame by frame (the reference block fed through its own ring buffer): a stream that starts
    in noise, frames back to back, symbols slipped in front of two of them; a stream already in lock; noise alone (every frame re-aligns somewhere).
    Same frames, same number of symbols taken per frame. (The reference driver only calls work2 while its ring holds two frames' worth, the
    entry point emits while a frame and its re-alignment symbols are there: it may deliver one or two frames more at the end of the input.)"""
    import ctypes as C
    from tests import dvbs2_util
    if not pyref.S2FrontRef.available() or not hasattr(C.CDLL(pyref.os.path.join(pyref._HERE, "_ref", "libsdref_dvbs2.so")), "sdref_s2_pl_sync"):
        pytest.skip("oracle/_ref/libsdref_dvbs2.so without the PL sync entry (rebuild with the reference tree)")
    probe = np.zeros(8, dtype=np.complex64)
    _, _, raw = pyref.s2_pl_sync_ref(slots, pilots, 0.6, probe, max_frames=1)
    nfr = 10 if slots < 360 else 5
    if kind == "slips":
        x = dvbs2_util.pl_stream(raw, (6 << 2) | pilots, nfr, seed=slots + pilots, lead=1234, glitches={3: 17, 6: raw // 2 + 5})
    elif kind == "locked":
        x = dvbs2_util.pl_stream(raw, (20 << 2) | 2, nfr, seed=9, lead=0)
    else:
        rng = np.random.default_rng(4)
        x = ((rng.standard_normal(nfr * raw) + 1j * rng.standard_normal(nfr * raw)) * 0.4).astype(np.complex64)
    want, wcons, _ = pyref.s2_pl_sync_ref(slots, pilots, 0.6, x)
    assert len(want) >= (3 if kind == "noise" else nfr - 3)  # in noise every frame re-aligns by up to a frame: about half as many come out
    d_x = to_dev(x.view(np.float32))
    cap = len(x) // raw + 2
    stride = raw + 6
    d_fr = zeros_dev(cap * stride * 2, np.float32)
    consumed = C.c_size_t(0)
    bp = np.full(cap, -1, dtype=np.int32)
    nf = capi.lib().sdhip_s2_pl_sync_dev(0, slots, pilots, 0.6, C.c_void_p(d_x[1]), len(x), C.c_void_p(d_fr[1]), stride, cap, C.byref(consumed), bp.ctypes.data_as(C.c_void_p))
    assert nf >= len(want), (nf, len(want), capi.last_error())
    got = from_dev(d_fr).view(np.complex64).reshape(cap, stride)[:nf, :raw]
    assert np.array_equal(bp[:len(want)] + raw, wcons), (bp[:nf].tolist(), (wcons - raw).tolist())
    assert np.array_equal(got[:len(want)].view(np.uint32), want.view(np.uint32))
    assert consumed.value == int(np.sum(bp[:nf] + raw)) and consumed.value <= len(x)
    if kind == "locked":
        assert np.all(bp[:nf] == 0)
    if kind == "slips":
        slips = {f: v for f, v in {0: 1234, 3: 17, 6: raw // 2 + 5}.items() if f < nf}  # (the 5-frame normal-FECFRAME case ends before the third)
        assert all(bp[f] == v for f, v in slips.items()) and np.count_nonzero(bp[:nf]) == len(slips)
    # max_frames is honoured and the call is restartable where it stopped
    d_fr2 = zeros_dev(cap * stride * 2, np.float32)
    nf2 = capi.lib().sdhip_s2_pl_sync_dev(0, slots, pilots, 0.6, C.c_void_p(d_x[1]), len(x), C.c_void_p(d_fr2[1]), stride, 2, C.byref(consumed), None)
    assert nf2 == 2 and consumed.value == int(np.sum(bp[:2] + raw))


@pytest.mark.parametrize("slots,pilots,kind", PLSYNC)
def test_pl_sync(capi, slots, pilots, kind):
    import torch

    def to_dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return (t, t.data_ptr())

    def zeros_dev(n, dt):
        t = torch.zeros(n, dtype={np.int8: torch.int8, np.int32: torch.int32, np.float32: torch.float32}[dt], device="cuda")
        return (t, t.data_ptr())

    check_pl_sync(capi, to_dev, lambda d: d[0].cpu().numpy(), zeros_dev, slots, pilots, kind)


def _dvbs2_ref_lib():
    import ctypes as C
    p = pyref.os.path.join(pyref._HERE, "_ref", "libsdref_dvbs2.so")
    if not pyref.os.path.exists(p) or not hasattr(C.CDLL(p), "sdref_s2_pll"):
        pytest.skip("oracle/_ref/libsdref_dvbs2.so without the PLL entries (rebuild with the reference tree)")
    return C.CDLL(p)


def check_atan2f(capi, to_dev, from_dev, zeros_dev):
    """The device restatement of glibc's atan2f / atanf (what complex_t::arg() calls in the frame PLL) == the host libm's atan2f, bit for bit:
    signal-like arguments, every quadrant, tiny / huge ratios, zeros, infinities, the x == 1 shortcut."""
    import ctypes as C
    lib = _dvbs2_ref_lib()
    rng = np.random.default_rng(12)
    n = 400000
    y = rng.standard_normal(n).astype(np.float32)
    x = rng.standard_normal(n).astype(np.float32)
    y[:50000] *= np.float32(1e-6)
    x[50000:100000] *= np.float32(1e-7)
    bits = rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)
    y[100000:200000] = bits.view(np.float32)
    x[150000:250000] = rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    sp = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1e-30, -1e30, 0.4375, 0.6875, 1.1875, 2.4375, 3.4e38], dtype=np.float32)
    k = len(sp)
    y[-k * k:] = np.repeat(sp, k)
    x[-k * k:] = np.tile(sp, k)
    ok = ~(np.isnan(x) | np.isnan(y))
    want = np.zeros(n, dtype=np.float32)
    lib.sdref_atan2f(y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), n, want.ctypes.data_as(C.c_void_p))
    d_y, d_x, d_o = to_dev(y), to_dev(x), zeros_dev(n, np.float32)
    assert capi.lib().sdhip_op_atan2f(0, C.c_void_p(d_y[1]), C.c_void_p(d_x[1]), n, C.c_void_p(d_o[1])) == 0
    got = from_dev(d_o)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))


def check_pll(capi, to_dev, from_dev, zeros_dev, modcod, short, pilots, nfr=5):
    """sdhip_s2_pll_dev == dvbs2::S2PLLBlock::work frame by frame (the reference block set up as the module sets it up, driven through its own
    streams): every symbol the block writes and the loop state behind the last frame, bit for bit -- in one call and in two (state carried by
    the caller)."""
    import ctypes as C
    from tests import dvbs2_util
    _dvbs2_ref_lib()
    ref = pyref.S2FrontRef()
    c = ref.cfg(modcod, short, pilots)
    probe = np.zeros(8, dtype=np.complex64)
    _, _, raw = pyref.s2_pl_sync_ref(c["slots"], pilots, 0.6, probe, max_frames=1)
    x = dvbs2_util.pl_stream(raw, (modcod << 2) | (short << 1) | pilots, nfr + 2, seed=modcod, lead=0, cfo=0.0004)
    fr, _, _ = pyref.s2_pl_sync_ref(c["slots"], pilots, 0.6, x)
    fr = fr[:nfr]
    want, walked, wst = pyref.s2_pll_ref(modcod, short, pilots, 0.002, fr)
    lut = pyref.s2_lut_phase_ref(modcod, short)
    d_in = to_dev(fr.view(np.float32))
    for cuts in ([0, nfr], [0, 2, nfr]):
        d_out = zeros_dev(fr.size * 2, np.float32)
        st = np.zeros(2, dtype=np.float32)
        for a, b in zip(cuts[:-1], cuts[1:]):
            off = a * fr.shape[1] * 8
            rc = capi.lib().sdhip_s2_pll_dev(0, modcod, short, pilots, 0.002, C.c_void_p(d_in[1] + off), C.c_void_p(d_out[1] + off), fr.shape[1], b - a,
                                             lut.ctypes.data_as(C.c_void_p), 256, st.ctypes.data_as(C.c_void_p))
            assert rc == walked, capi.last_error()
        got = from_dev(d_out).view(np.complex64).reshape(fr.shape)
        assert np.array_equal(got[:, :walked].view(np.uint32), want[:, :walked].view(np.uint32))
        assert np.array_equal(st.view(np.uint32), wst.view(np.uint32))
    assert abs(float(wst[1]) - 0.0004) < 1e-4  # the loop sits on the stream's offset
    assert walked == (c["slots"] + 1) * 90 + (36 if pilots else 0)


def _torch_helpers():
    import torch

    def to_dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return (t, t.data_ptr())

    def zeros_dev(n, dt):
        t = torch.zeros(n, dtype={np.int8: torch.int8, np.int32: torch.int32, np.float32: torch.float32, np.uint8: torch.uint8}[dt], device="cuda")
        return (t, t.data_ptr())

    return to_dev, (lambda d: d[0].cpu().numpy()), zeros_dev


def test_atan2f(capi):
    check_atan2f(capi, *_torch_helpers())


@pytest.mark.parametrize("modcod,short,pilots", [(4, 1, 0), (13, 1, 0), (20, 1, 0), (6, 1, 1)])
def test_pll(capi, modcod, short, pilots):
    check_pll(capi, *_torch_helpers(), modcod, short, pilots)


def check_symbols_to_bbframes(capi, to_dev, from_dev, zeros_dev, nfr=4, via_baseband=None):
    """The DVB-S2 receive chain behind the clock recovery on the device, entry by entry -- PL synchroniser, frame PLL, soft demapper stage, LDPC,
    repack, BCH, BB descrambler -- against the reference's own classes chained the same way (DVBS2DemodModule's blocks and process_s2):
    short QPSK 1/2 frames carrying BCH + LDPC encoded random BBFRAMEs, a leading stretch of noise, a carrier offset: identical BBFRAMEs, and
    they are the transmitted ones."""
    import ctypes as C
    from tests import dvbs2_util
    _dvbs2_ref_lib()
    modcod, short, rate = 4, 1, "1/2"
    rc_ = capi.S2_RATES[rate]
    front, fec = pyref.S2FrontRef(), pyref.Dvbs2Ref(False)
    c = front.cfg(modcod, short, 0)
    n, k = fec.dims(short, rc_)
    kb = fec.bch_kbch(short, rc_)
    rng = np.random.default_rng(21)
    bb = np.zeros((nfr, k // 8), dtype=np.uint8)
    bb[:, :kb // 8] = rng.integers(0, 256, (nfr, kb // 8), dtype=np.uint8)
    scr = fec.bb_descramble(short, rc_, bb.copy())           # the BB scrambler is its own inverse
    cw = dvbs2_util.encode(short, rc_, np.unpackbits(fec.bch_encode(short, rc_, scr.copy()), axis=1))
    raw = (c["slots"] + 1) * 90
    x = dvbs2_util.pl_stream_from_bits(cw, raw, (modcod << 2) | (short << 1), seed=5, lead=0 if via_baseband else 777, cfo=0.0003, esn0_db=9.0)
    xref = x
    if via_baseband:
        # the clean symbol stream is pulse-shaped to 2.5 samples per symbol with a timing offset, a carrier offset and noise (synth.modulate); the
        # reference recovers the symbols with its AGC, RRC filter and M&M blocks, the device with the front-end handle (via_baseband = "exact":
        # the same symbols bit for bit; "chunk": the chunk-parallel schedule's)
        from satdump_amd import synth
        clean = dvbs2_util.pl_stream_from_bits(cw, raw, (modcod << 2) | (short << 1), seed=5, lead=0, cfo=0.0, esn0_db=80.0) * 1.5
        spec = synth.SynthSpec(constellation="qpsk", samplerate=2.5e6, symbolrate=1e6, rrc_alpha=0.35, amplitude=0.5, cfo_hz=60.0, esn0_db=7.0, seed=3, timing_offset=0.3)
        bbx, _ = synth.modulate(clean.astype(np.complex128), spec)
        orc = pyref.best()
        xref = orc.block(3, [2.5, (8.7e-3) ** 2 / 4, 0.5, 8.7e-3, 0.005], orc.block(1, [2.5e6, 1e6, 0.35, 31], orc.block(0, [1e-3, 1.0, 1.0, 65536.0], bbx)))
        dem = capi.PskDemod(capi.demod_cfg(samplerate=2.5e6, symbolrate=1e6, constellation="qpsk", rrc_alpha=0.35, rrc_taps=31, agc_rate=1e-3, pll_bw=0.005,
                                           exact=1 if via_baseband == "exact" else 0, chunk_len=0 if via_baseband == "exact" else 8192), front_only=True)
        d_bb = to_dev(bbx.view(np.float32))
        d_so, d_sy = zeros_dev(2 * len(bbx) + 64, np.int8), zeros_dev(2 * (len(bbx) + 64), np.float32)
        ns = dem.process_dev(d_bb[1], len(bbx), capi.FMT_CF32, d_so[1], 2 * len(bbx) + 64, d_sy[1], len(bbx) + 64)
        x = from_dev(d_sy)[: 2 * (ns // 2)].view(np.complex64).copy()
        if via_baseband == "exact":
            assert len(x) == len(xref) and np.array_equal(x.view(np.uint32), xref.view(np.uint32))
    # ---- reference chain
    fr, _, _ = pyref.s2_pl_sync_ref(c["slots"], 0, 0.6, xref)
    rp, walked, _ = pyref.s2_pll_ref(modcod, short, 0, 0.002, fr)
    soft, _ = front.bb_to_soft(modcod, short, 0, rp)
    dec, _tr = fec.ldpc_decode(short, rc_, soft.copy(), 25)
    packed = np.packbits((dec < 0).astype(np.uint8), axis=1)[:, :k // 8]
    wfix, wcorr = fec.bch_decode(short, rc_, packed.copy())
    want = fec.bb_descramble(short, rc_, wfix.copy())
    # what the reference delivers: transmitted frames, in order (from baseband the first ones are lost to the AGC / clock loop's acquisition)
    sent = {bytes(r[:kb // 8]): i for i, r in enumerate(bb)}
    hits = [sent.get(bytes(r[:kb // 8]), -1) for r in want]
    found = [h for h in hits if h >= 0]
    assert found == sorted(found) and len(found) >= (3 if via_baseband else nfr - 1), hits
    # ---- device chain
    L = capi.lib()
    d_x = to_dev(x.view(np.float32))
    cap = nfr + 2
    stride = raw + 6
    d_fr, d_pl = zeros_dev(cap * stride * 2, np.float32), zeros_dev(cap * stride * 2, np.float32)
    consumed = C.c_size_t(0)
    nf = L.sdhip_s2_pl_sync_dev(0, c["slots"], 0, 0.6, C.c_void_p(d_x[1]), len(x), C.c_void_p(d_fr[1]), stride, cap, C.byref(consumed), None)
    if via_baseband != "chunk":
        assert nf >= len(want)
        nf = len(want)
    st = np.zeros(2, dtype=np.float32)
    lutp, lutb = pyref.s2_lut_phase_ref(modcod, short), front.lut(modcod, short)
    assert L.sdhip_s2_pll_dev(0, modcod, short, 0, 0.002, C.c_void_p(d_fr[1]), C.c_void_p(d_pl[1]), stride, nf, lutp.ctypes.data_as(C.c_void_p), 256,
                              st.ctypes.data_as(C.c_void_p)) == walked
    d_soft = zeros_dev(nf * n, np.int8)
    assert L.sdhip_s2_bb_to_soft_dev(0, modcod, short, 0, C.c_void_p(d_pl[1]), stride, nf, lutb.ctypes.data_as(C.c_void_p), 256, C.c_void_p(d_soft[1]), None) == n
    ldpc = capi.LdpcDecoder(framesize=short, rate=rate, batch=1)
    bch = capi.BchDecoder(framesize=short, rate=rate)
    d_tr = zeros_dev(nf, np.int32)
    ldpc.decode_dev(d_soft[1], nf, 25, d_tr[1])
    d_pack = zeros_dev(nf * (k // 8), np.uint8)
    d_corr = zeros_dev(nf, np.int32)
    bch.pack_dev(d_soft[1], n, nf, d_pack[1], k // 8)
    bch.decode_dev(d_pack[1], nf, k // 8, d_corr[1])
    bch.descramble_dev(d_pack[1], nf, k // 8)
    got = from_dev(d_pack).reshape(nf, k // 8)
    if via_baseband == "chunk":
        # other float symbols (inside the clock recovery's floor; its rare symbol slips need not fall where the sequential loop's do): the
        # contract here is the decoders' output -- transmitted frames, in order, about as many as the reference recovers
        ghits = [sent.get(bytes(r[:kb // 8]), -1) for r in got]
        gfound = [h for h in ghits if h >= 0]
        assert gfound == sorted(gfound) and len(gfound) >= 3 and len(gfound) >= len(found) - 2, (ghits, hits)
    else:
        assert np.array_equal(from_dev(d_corr), wcorr) and np.array_equal(got, want)


def test_symbols_to_bbframes(capi):
    check_symbols_to_bbframes(capi, *_torch_helpers())


@pytest.mark.parametrize("front", ["exact", "chunk"])
def test_baseband_to_bbframes(capi, front):
    """The whole DVB-S2 receive path on the device, baseband samples in, BBFRAMEs out: front end (AGC, RRC filter, clock recovery), PL synchroniser,
    frame PLL, soft demapper stage, LDPC, BCH, BB descrambler -- against the reference's blocks and classes chained the same way."""
    check_symbols_to_bbframes(capi, *_torch_helpers(), nfr=10, via_baseband=front)


def check_dvbs2_demod_mirror(capi, make_mem):
    """satdump_amd.dvbs2.DVBS2Demod -- the module's parameter keys, baseband in, BBFRAMEs out, carry-over between calls -- against the reference's
    blocks and classes chained the same way: identical BBFRAMEs in exact mode, whether the samples arrive in one call or in five ragged ones;
    the module's error messages for missing parameters; the frequency feedback refused in exact mode (it runs on thread timing in the reference).
    Since round 4 the mirror is a thin face of the C++ engine handle (sdhip_dvbs2_demod_*)."""
    from satdump_amd import dvbs2, synth
    from tests import dvbs2_util
    _dvbs2_ref_lib()
    modcod, short, rc_ = 4, 1, 3
    front, fec = pyref.S2FrontRef(), pyref.Dvbs2Ref(False)
    c = front.cfg(modcod, short, 0)
    n, k = fec.dims(short, rc_)
    kb = fec.bch_kbch(short, rc_)
    nfr = 10
    rng = np.random.default_rng(21)
    bb = np.zeros((nfr, k // 8), dtype=np.uint8)
    bb[:, :kb // 8] = rng.integers(0, 256, (nfr, kb // 8), dtype=np.uint8)
    cw = dvbs2_util.encode(short, rc_, np.unpackbits(fec.bch_encode(short, rc_, fec.bb_descramble(short, rc_, bb.copy())), axis=1))
    raw = (c["slots"] + 1) * 90
    clean = dvbs2_util.pl_stream_from_bits(cw, raw, (modcod << 2) | (short << 1), seed=5, lead=0, cfo=0.0, esn0_db=80.0) * 1.5
    spec = synth.SynthSpec(constellation="qpsk", samplerate=2.5e6, symbolrate=1e6, rrc_alpha=0.35, amplitude=0.5, cfo_hz=60.0, esn0_db=7.0, seed=3, timing_offset=0.3)
    bbx, _ = synth.modulate(clean.astype(np.complex128), spec)
    params = {"samplerate": 2.5e6, "symbolrate": 1e6, "rrc_alpha": 0.35, "pll_bw": 0.002, "modcod": modcod, "shortframes": True, "agc_rate": 1e-3,
              "clock_alpha": 8.7e-3, "freq_prop_factor": 0.0, "ldpc_trials": 25}
    # ---- the reference chain
    orc = pyref.best()
    xref = orc.block(3, [2.5, (8.7e-3) ** 2 / 4, 0.5, 8.7e-3, 0.005], orc.block(1, [2.5e6, 1e6, 0.35, 31], orc.block(0, [1e-3, 1.0, 1.0, 65536.0], bbx)))
    fr, _, _ = pyref.s2_pl_sync_ref(c["slots"], 0, 0.6, xref)
    rp, _, _ = pyref.s2_pll_ref(modcod, short, 0, 0.002, fr)
    soft, _ = front.bb_to_soft(modcod, short, 0, rp)
    dec, _ = fec.ldpc_decode(short, rc_, soft.copy(), 25)
    wfix, _ = fec.bch_decode(short, rc_, np.packbits((dec < 0).astype(np.uint8), axis=1)[:, :k // 8].copy())
    want = fec.bb_descramble(short, rc_, wfix.copy())[:, :kb // 8]
    sent = {bytes(r[:kb // 8]): i for i, r in enumerate(bb)}
    assert sum(bytes(r) in sent for r in want) >= 3
    # ---- the mirror, one call and five ragged calls
    lut_b, lut_p = front.lut(modcod, short), pyref.s2_lut_phase_ref(modcod, short)
    for cuts in ([0, len(bbx)], [0, 5000, 5001, 77777, 150000, len(bbx)]):
        dem = dvbs2.DVBS2Demod(params, lut_b, lut_p, mem=make_mem(), capi=capi, exact=True)
        assert dem.bbframe_bytes == kb // 8
        got = np.concatenate([dem.process(bbx[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
        assert len(got) >= len(want) - 1 and np.array_equal(got[:len(want)], want[:len(got)])
        assert dem.stats["pls"] is not None and dem.stats["frames"] == len(got)
    for missing, msg in (("rrc_alpha", "RRC Alpha parameter must be present!"), ("pll_bw", "PLL BW parameter must be present!"), ("modcod", "MODCOD parameter must be present!")):
        with pytest.raises(ValueError, match=msg.replace("!", ".")):
            dvbs2.DVBS2Demod({k2: v for k2, v in params.items() if k2 != missing}, lut_b, lut_p, mem=make_mem(), capi=capi)
    with pytest.raises(capi.SdhipError, match="freq_prop_factor must be 0"):  # exact mode cannot reproduce a thread-timed feedback
        dvbs2.DVBS2Demod(dict(params, freq_prop_factor=0.01), lut_b, lut_p, mem=make_mem(), capi=capi, exact=True)
    with pytest.raises(ValueError, match="32APSK"):
        dvbs2.DVBS2Demod(dict(params, modcod=25), lut_b, lut_p, mem=make_mem(), capi=capi)



def test_dvbs2_demod_mirror(capi):
    from satdump_amd import dvbs2
    check_dvbs2_demod_mirror(capi, dvbs2.TorchMem)


def _s2_reference_chain(modcod, short, x_syms, trials=25, loop_bw=0.002):
    """DVBS2DemodModule's blocks behind the clock recovery, chained the way the module chains them: BBFRAMEs (kbch / 8 bytes each), LDPC trials, BCH results,
    the PLL's output frames."""
    front, fec = pyref.S2FrontRef(), pyref.Dvbs2Ref(False)
    c = front.cfg(modcod, short, 0)
    rc_ = c["rate"]
    n, k = fec.dims(short, rc_)
    kb = fec.bch_kbch(short, rc_)
    fr, _, _ = pyref.s2_pl_sync_ref(c["slots"], 0, 0.6, x_syms)
    rp, walked, st = pyref.s2_pll_ref(modcod, short, 0, loop_bw, fr)
    soft, _ = front.bb_to_soft(modcod, short, 0, rp)
    dec, tr = fec.ldpc_decode(short, rc_, soft.copy(), trials)
    fix, corr = fec.bch_decode(short, rc_, np.packbits((dec < 0).astype(np.uint8), axis=1)[:, :k // 8].copy())
    return fec.bb_descramble(short, rc_, fix.copy())[:, :kb // 8], tr, corr, fr, rp, st


def check_pll_parallel(capi, to_dev, from_dev, zeros_dev, modcod, short, esn0_db, nfr, lane_len=0):
    """The frame-parallel schedule of the frame PLL (sdhip_s2_pll_frames_dev, mode 2 = a new stream) against the reference's serial loop on the same
    synchronised frames. What it promises is the DECODERS' output, not the loop's symbols to 1e-5: the loop's detector is a 256 x 256 table
    (piecewise-constant feedback), two trajectories on the same symbols stay ~1e-2 (8PSK) of a symbol apart for good (tools/s2_pll_frame_study.py,
    DESIGN.md 4b) -- so: the same hard decisions out of the LDPC decoder for every frame, soft bits equal on > 80 % (the rest a table cell or two apart), the end state on the same
    stable point, and lanes actually ran in parallel without wholesale re-runs."""
    import ctypes as C
    from satdump_amd import synth_dvbs2 as sd
    _dvbs2_ref_lib()
    c = sd.modcod_cfg(modcod, short)
    bb = sd.bbframes_random(short, c["rate"], nfr, seed=3)
    fr = sd.plframes(modcod, short, bb)
    raw = fr.shape[1]
    x = sd.symbol_stream(fr, seed=5, lead=0, cfo=0.0004, esn0_db=esn0_db, amplitude=0.7 if c["bits"] != 2 else 2.0 / 3.0)
    frames = np.ascontiguousarray(x[: nfr * raw].reshape(nfr, raw))
    want, walked, wst = pyref.s2_pll_ref(modcod, short, 0, 0.002, frames)
    lut = pyref.s2_lut_phase_ref(modcod, short)
    d_in, d_out = to_dev(frames.view(np.float32)), zeros_dev(frames.size * 2, np.float32)
    st = np.zeros(2, dtype=np.float32)
    stats = (C.c_uint * 4)()
    old = {k: os.environ.get(k) for k in ("SDHIP_S2PLL_ACQ", "SDHIP_S2PLL_L")}
    os.environ["SDHIP_S2PLL_ACQ"] = str(3 * raw)
    if lane_len:
        os.environ["SDHIP_S2PLL_L"] = str(lane_len)
    try:
        rc = capi.lib().sdhip_s2_pll_frames_dev(0, modcod, short, 0, 0.002, C.c_void_p(d_in[1]), C.c_void_p(d_out[1]), raw, nfr, lut.ctypes.data_as(C.c_void_p), 256,
                                                st.ctypes.data_as(C.c_void_p), 2, stats)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert rc == walked, capi.last_error()
    got = from_dev(d_out).view(np.complex64).reshape(frames.shape)
    lanes, rerun, forced, serial = list(stats)
    assert serial == 3 and lanes >= 2 and forced == 0 and rerun <= max(1, lanes // 8), list(stats)
    # the serial stretch is the reference's loop bit for bit
    assert np.array_equal(got[:3, :walked].view(np.uint32), want[:3, :walked].view(np.uint32))
    err = np.abs(got[:, :walked] - want[:, :walked]) / np.sqrt(np.mean(np.abs(want[:, :walked]) ** 2))
    assert err.max() < 0.3 and np.quantile(err, 0.99) < 0.1, (err.max(), np.quantile(err, 0.99))  # (2 048-step lanes: a good part of every lane is its settling stretch)
    dph = (float(st[0]) - float(wst[0]) + np.pi) % (2 * np.pi) - np.pi
    assert abs(dph) < 0.08 and abs(float(st[1]) - float(wst[1])) < 1e-4, (st, wst)
    front, fec = pyref.S2FrontRef(), pyref.Dvbs2Ref(False)
    s1, _ = front.bb_to_soft(modcod, short, 0, want)
    s2, _ = front.bb_to_soft(modcod, short, 0, got)
    assert (s1 == s2).mean() > 0.8  # the others a table cell or two apart (no bound on a single one: the table's clamp halves values beyond 127)
    d1, t1 = fec.ldpc_decode(short, c["rate"], s1.copy(), 25)
    d2, t2 = fec.ldpc_decode(short, c["rate"], s2.copy(), 25)
    # frames both decoders converge on: the same code word. (The reference's decoder reports "not converged" on valid code words of most SHORT codes --
    # tests/dvbs2_util.py -- and what it leaves then depends on the last soft bit: those frames are compared behind the BCH decoder, which is where the
    # module takes its BBFRAMEs from.)
    conv = (t1 >= 0) & (t2 >= 0)
    assert np.array_equal((d1 < 0)[conv], (d2 < 0)[conv])
    n, k = fec.dims(short, c["rate"])
    b1, c1 = fec.bch_decode(short, c["rate"], np.packbits((d1 < 0).astype(np.uint8), axis=1)[:, :k // 8].copy())
    b2, c2 = fec.bch_decode(short, c["rate"], np.packbits((d2 < 0).astype(np.uint8), axis=1)[:, :k // 8].copy())
    okf = (c1 >= 0) & (c2 >= 0)
    assert okf.sum() >= nfr - 1 and np.array_equal(b1[okf], b2[okf]) and np.array_equal(c1 >= 0, c2 >= 0)


@pytest.mark.parametrize("modcod,short,esn0_db,nfr,lane_len", [(12, 1, 9.0, 16, 0), (12, 1, 9.0, 10, 1500), (6, 1, 6.0, 12, 0), (13, 0, 9.5, 6, 0)])
def test_pll_parallel(capi, modcod, short, esn0_db, nfr, lane_len):
    check_pll_parallel(capi, *_torch_helpers(), modcod, short, esn0_db, nfr, lane_len)


def _s2_baseband(modcod, short, nfr, esn0_db, seed=3, cfo_hz=0.0, sps=2.0, alpha=0.2):
    """nfr PLFRAMEs of random BBFRAMEs as baseband samples (complex64) at sps samples per symbol, and the BBFRAMEs. No carrier offset by default:
    the reference's frame PLL, cold-started on the front end's settling transient, does not pull 8PSK in from even 10 Hz at 1 Msym/s within a
    dozen frames (measured on the compiled reference; in the module that is what freq_prop_factor and patience are for) -- and a loop that is
    not locked has no output to compare."""
    from satdump_amd import synth, synth_dvbs2 as sd
    c = sd.modcod_cfg(modcod, short)
    bb = sd.bbframes_random(short, c["rate"], nfr, seed=seed)
    fr = sd.plframes(modcod, short, bb)
    rng = np.random.default_rng(seed + 1)
    tail = (rng.standard_normal(3 * fr.shape[1]) + 1j * rng.standard_normal(3 * fr.shape[1])) * 0.3
    clean = np.concatenate([fr.reshape(-1), tail])
    spec = synth.SynthSpec(constellation="qpsk", samplerate=sps * 1e6, symbolrate=1e6, rrc_alpha=alpha, amplitude=0.5, cfo_hz=cfo_hz, esn0_db=esn0_db, seed=seed, timing_offset=0.3)
    bbx, _ = synth.modulate(clean, spec)
    return bbx, bb


def check_dvbs2_engine(capi, make_mem, modcod=12, short=1, nfr=16, esn0_db=10.0, freq_prop=0.0, cuts=None, acq=None, cfo_hz=0.0, min_handover=0.6):
    """The DVB-S2 demodulator handle (sdhip_dvbs2_demod_*) in its DEFAULT schedules -- chunk-parallel front end, frame-parallel PLL -- on 8PSK frames,
    baseband in, BBFRAMEs out, against the reference's blocks and classes chained the way the module chains them: the same BBFRAMEs in the same order
    (the contract of the parallel schedules: the decoders' output), all of them transmitted ones; with freq_prop_factor (the reference's feedback runs
    on thread timing: no frame-for-frame reference exists) every frame out is a transmitted one, in order, no fewer than the reference chain finds
    without the feedback, and the rotator ends up carrying the offset."""
    from satdump_amd import dvbs2
    _dvbs2_ref_lib()
    bbx, bb = _s2_baseband(modcod, short, nfr, esn0_db, cfo_hz=cfo_hz)
    sent = {bytes(r): i for i, r in enumerate(bb)}
    orc = pyref.best()
    xref = orc.block(3, [2.0, (1.7e-3) ** 2 / 4, 0.5, 1.7e-3, 0.005], orc.block(1, [2e6, 1e6, 0.2, 31], orc.block(0, [1e-2, 1.0, 1.0, 65536.0], bbx)))
    want, _, _, _, _, _ = _s2_reference_chain(modcod, short, xref, trials=25)
    whits = [sent.get(bytes(r), -1) for r in want]
    wfound = [h for h in whits if h >= 0]
    assert len(wfound) >= nfr - 4 and wfound == sorted(wfound), whits
    front = pyref.S2FrontRef()
    lut_b, lut_p = front.lut(modcod, short), pyref.s2_lut_phase_ref(modcod, short)
    params = {"samplerate": 2e6, "symbolrate": 1e6, "rrc_alpha": 0.2, "pll_bw": 0.002, "modcod": modcod, "shortframes": bool(short), "freq_prop_factor": freq_prop, "ldpc_trials": 25}
    old = os.environ.get("SDHIP_S2PLL_ACQ")
    if acq:
        os.environ["SDHIP_S2PLL_ACQ"] = str(acq)
    try:
        dem = dvbs2.DVBS2Demod(params, lut_b, lut_p, mem=make_mem(), capi=capi)
        cuts = cuts or [0, len(bbx)]
        parts, seen = [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts.append(dem.process(bbx[a:b]))
            seen.append(dem.stats)
        got = np.concatenate(parts)
    finally:
        if old is None:
            os.environ.pop("SDHIP_S2PLL_ACQ", None)
        else:
            os.environ["SDHIP_S2PLL_ACQ"] = old
    st = dem.stats
    ghits = [sent.get(bytes(r), -1) for r in got]
    gfound = [h for h in ghits if h >= 0]
    assert gfound == sorted(gfound) and len(gfound) >= len(wfound) - 1, (ghits, whits)
    assert st["pll_lanes"] >= 2 and st["pll_forced"] <= st["pll_lanes"] // 4, st  # (the noise behind the stream certifies nothing: its lanes end up forced)
    if len(cuts) > 2:  # the module's statistics describe the LAST frame: in mid-stream that is a frame of the signal (behind the stream, noise)
        assert any(q["detected_modcod"] == modcod and q["detected_shortframes"] == short and q["snr"] > 3.0 for q in seen[:-1]), seen
    if freq_prop == 0.0:
        # frame for frame the reference's output from the first frame both deliver (the parallel front end may lock a frame earlier or later)
        k0 = next(i for i, h in enumerate(ghits) if h >= 0 and h in whits)
        r0 = whits.index(ghits[k0])
        m = min(len(got) - k0, len(want) - r0)
        good = np.array([h >= 0 for h in whits[r0:r0 + m]])  # frames of noise behind the stream: two decoders that do not converge owe each other nothing
        assert good.sum() >= nfr - 5 and np.array_equal(got[k0:k0 + m][good], want[r0:r0 + m][good])
    else:
        q = seen[-2]  # behind the last call of the signal proper
        # the rotator has taken the offset over (most of it at the larger factors; 1 - (1 - factor)^frames of it in any case)
        assert -1.1 * cfo_hz < q["freq_hz"] < -min_handover * cfo_hz and abs(q["pll_freq"]) < 2 * np.pi * cfo_hz / 1e6, seen
    return st


def test_dvbs2_engine_parallel(capi):
    from satdump_amd import dvbs2
    st = check_dvbs2_engine(capi, dvbs2.TorchMem, modcod=13, short=0, nfr=10, esn0_db=10.0, acq=2 * 21690)
    assert st["pll_serial_frames"] == 2


def test_dvbs2_engine_parallel_ragged_calls(capi):
    from satdump_amd import dvbs2
    check_dvbs2_engine(capi, dvbs2.TorchMem, modcod=12, short=1, nfr=24, esn0_db=10.0, cuts=[0, 40001, 40002, 123457, 200000, 24 * 5490 * 2 + 3 * 5490 * 2], acq=3 * 5490)


def test_dvbs2_engine_freq_prop(capi):
    from satdump_amd import dvbs2
    check_dvbs2_engine(capi, dvbs2.TorchMem, modcod=4, short=1, nfr=40, esn0_db=7.0, freq_prop=0.05, acq=3 * 8190, cfo_hz=50.0,
                       cuts=[0] + [8190 * 2 * 5 * k for k in range(1, 9)] + [43 * 8190 * 2])


def test_dvbs2_engine_freq_prop_hand_over(capi):
    """the symbols waiting in the PL synchroniser's ring at a hand-over are turned on at the new rate (they reached the loop with a +d / -d frequency
    step before). A larger offset, the module's default factor 0.01, a hand-over every two frames: every frame the reference chain finds (without the feedback)
    comes out, in order, and the rotator carries 1 - 0.99^frames of the offset."""
    from satdump_amd import dvbs2
    check_dvbs2_engine(capi, dvbs2.TorchMem, modcod=4, short=1, nfr=40, esn0_db=7.0, freq_prop=0.01, acq=3 * 8190, cfo_hz=120.0,
                       cuts=[0] + [8190 * 2 * 2 * k for k in range(1, 21)] + [43 * 8190 * 2], min_handover=0.2)



def check_bb_to_soft_golden(capi, to_dev, from_dev, zeros_dev):
    """The committed fixture tests/golden/s2_bb_to_soft.npz (written by make_golden.py from the compiled reference): stored PLFRAMEs and the
    reference's demapper table -> its PLS indices and soft bits, byte for byte. Needs no reference build at run time."""
    import ctypes as C
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s2_bb_to_soft.npz"))
    fr, lut = g["frames"], np.ascontiguousarray(g["lut"])
    nframes, nsoft = g["soft"].shape
    d_fr = to_dev(fr.view(np.float32))
    d_soft = zeros_dev(nframes * nsoft, np.int8)
    d_pls = zeros_dev(nframes, np.int32)
    rc = capi.lib().sdhip_s2_bb_to_soft_dev(0, int(g["modcod"]), int(g["shortframes"]), int(g["pilots"]), C.c_void_p(d_fr[1]), fr.shape[1], nframes,
                                            lut.ctypes.data_as(C.c_void_p), lut.shape[0], C.c_void_p(d_soft[1]), C.c_void_p(d_pls[1]))
    assert rc == nsoft, capi.last_error()
    assert np.array_equal(from_dev(d_pls), g["pls"]) and np.array_equal(from_dev(d_soft).reshape(nframes, nsoft), g["soft"])


def test_bb_to_soft_golden(capi):
    import torch

    def to_dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return (t, t.data_ptr())

    def zeros_dev(n, dt):
        t = torch.zeros(n, dtype={np.int8: torch.int8, np.int32: torch.int32}[dt], device="cuda")
        return (t, t.data_ptr())

    check_bb_to_soft_golden(capi, to_dev, lambda d: d[0].cpu().numpy(), zeros_dev)


def test_bb_to_soft_refusals(capi):
    """32APSK (no demapper table in the reference) and MODCODs outside the table come back as errors with the reference's wording."""
    import ctypes as C
    lut = np.zeros((256, 256, 5), dtype=np.int8)
    for modcod, msg in ((24, "32APSK"), (0, "MODCOD cannot be <= 0!"), (29, "MODCOD not (yet?) supported!")):
        rc = capi.lib().sdhip_s2_bb_to_soft_dev(0, modcod, 0, 0, None, 40000, 1, lut.ctypes.data_as(C.c_void_p), 256, None, None)
        assert rc < 0 and msg in capi.last_error()


def test_errors(capi):
    with pytest.raises(capi.SdhipError):
        capi.LdpcDecoder(framesize=0, rate="7/8")   # no LDPC table (bbframe_ldpc.cpp:30-69 has no case for it)
    with pytest.raises(capi.SdhipError):
        capi.LdpcDecoder(framesize=1, rate="9/10")
    dec = capi.LdpcDecoder(framesize=1, rate="1/2", batch=16)
    with pytest.raises(capi.SdhipError):
        dec.decode(np.zeros((3, 16200), dtype=np.int8))  # not a whole number of batches


# ---------------------------------------------------------------------------------------------------- dvbs2_ts_extractor (round 6)
def _crc8_tab():
    tab = np.zeros(256, dtype=np.uint8)
    for i in range(256):
        r, crc = i, 0
        for j in range(7, -1, -1):
            if ((1 if r & (1 << j) else 0) ^ (1 if crc & 0x80 else 0)):
                crc = ((crc << 1) ^ 0xD5) & 0xFFFF
            else:
                crc = (crc << 1) & 0xFFFF
        tab[i] = crc & 0xFF
    return tab


def _hdr_crc_bits(hdr10):
    crc = 0
    for n in range(80):
        b = ((hdr10[n // 8] >> (7 - (n % 8))) & 1) ^ (crc & 1)
        crc >>= 1
        if b:
            crc ^= 0xAB
    return crc


def ts_bbframes(kbch, nframes, seed=1, dfls=None, bad_hdr=(), bad_syncd=(), corrupt_packets=(), start_skew=0):
    """BBFRAMEs the way a DVB-S2 modulator in TS mode builds them (EN 302 307 5.1): a continuous stream of 188-byte packets whose sync byte is replaced by the CRC-8
    of the previous packet's 187 other bytes, cut into data fields of dfls[k] bits (default: the whole frame), each behind a 10-byte header (MATYPE, UPL, DFL, SYNC,
    SYNCD = bits from the data field's start to the first sync/CRC byte in it, CRC-8). Returns (frames [n][kbch / 8], the packets as transmitted [m][188])."""
    rng = np.random.default_rng(seed)
    tab = _crc8_tab()
    fb = kbch // 8
    dfls = list(dfls) if dfls is not None else [kbch - 80] * nframes
    total = sum(d // 8 for d in dfls)
    npk = total // 188 + 3
    pk = rng.integers(0, 256, (npk, 188), dtype=np.uint8)
    pk[:, 0] = 0x47
    stream = np.zeros(npk * 188, dtype=np.uint8)
    for j in range(npk):
        stream[188 * j + 1:188 * j + 188] = pk[j, 1:]
        crc = 0
        if j > 0:
            for v in pk[j - 1, 1:]:
                crc = tab[v ^ crc]
            stream[188 * j] = crc ^ (0x55 if (j - 1) in corrupt_packets else 0)  # (a wrong CRC byte = a packet the receiver flags)
        else:
            stream[0] = 0
    frames = np.zeros((nframes, fb), dtype=np.uint8)
    at = start_skew  # position in `stream` of the next data-field byte
    for k in range(nframes):
        n = dfls[k] // 8
        syncd = (-at) % 188  # bytes to the next sync/CRC byte
        if k in bad_syncd:
            syncd = (syncd + 5) % 188
        h = np.zeros(10, dtype=np.uint8)
        h[0], h[1] = 0xF0, 0x00
        h[2], h[3] = (188 * 8) >> 8, (188 * 8) & 0xFF
        h[4], h[5] = dfls[k] >> 8, dfls[k] & 0xFF
        h[6] = 0x47
        h[7], h[8] = (syncd * 8) >> 8, (syncd * 8) & 0xFF
        for c in range(256):
            h[9] = c
            if _hdr_crc_bits(h) == 0:
                break
        if k in bad_hdr:
            h[9] ^= 0x3C
        frames[k, :10] = h
        frames[k, 10:10 + n] = stream[at:at + n]
        frames[k, 10 + n:] = rng.integers(0, 256, fb - 10 - n, dtype=np.uint8)  # padding behind the data field
        at += n
    return frames, pk


def _ts_run(capi, frames, kbch, cuts=None):
    h = capi.lib().sdhip_s2_ts_create(0, kbch)
    assert h, capi.last_error()
    capi.lib().sdhip_s2_ts_process.restype = C.c_int64
    out = []
    cuts = cuts or [0, len(frames)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        f = np.ascontiguousarray(frames[a:b])
        cap = (b - a) * (kbch // 8 // 188 + 2) + 8
        o = np.zeros((cap, 188), dtype=np.uint8)
        n = capi.lib().sdhip_s2_ts_process(C.c_void_p(h), f.ctypes.data_as(C.c_void_p), C.c_int(b - a), o.ctypes.data_as(C.c_void_p), C.c_size_t(cap))
        assert n >= 0, capi.last_error()
        out.append(o[:n])
    capi.lib().sdhip_s2_ts_destroy(C.c_void_p(h))
    return np.concatenate(out) if out else np.zeros((0, 188), dtype=np.uint8)


TS_CASES = [
    ("full_frames", dict(nframes=40)),                                                     # the data field fills the frame: packets span frames all the time
    ("short_fields", dict(nframes=60, dfls=[8 * v for v in ([700, 96, 187, 188, 189, 1500, 40, 8, 375, 376] * 6)])),  # fields shorter than a packet, ends ON a packet end
    ("header_crc", dict(nframes=40, bad_hdr=(5, 6, 20))),                                  # lost frames: resynchronisation from SYNCD, the packet in flight dropped
    ("syncd_off", dict(nframes=30, bad_syncd=(7, 19))),                                    # a SYNCD that contradicts the parser's count: out of sync from the NEXT frame
    ("payload_errors", dict(nframes=30, corrupt_packets=(3, 4, 50, 51, 52, 200))),         # the transport error indicator (and where the parser loses it)
    ("mid_stream", dict(nframes=25, start_skew=77)),                                       # the recording starts inside a packet
    ("aligned_ends", dict(nframes=48, dfls=[188 * 8 * 3, 188 * 8 * 3 + 8 * 187, 8 * 1, 188 * 8 * 2] * 12, corrupt_packets=tuple(range(0, 120, 2)))),  # CRC bytes that open a frame
]


@pytest.mark.parametrize("name,kw", TS_CASES)
def test_s2_ts_extractor(capi, name, kw):
    """The step behind the BBFRAMEs (plugins/dvb_support/dvbs2/module_s2_ts_extractor.cpp -> dvbs2::BBFrameTSParser): the packets the engine gathers on the device
    (sdhip_s2_ts_process: header walk on the host, packet gather + CRC-8 + error indicator per packet on the device) against the reference's parser compiled in place,
    byte for byte -- sync loss and recovery, fields shorter than a packet, the error indicator and the cases in which the parser itself drops it -- in one call and in
    ragged calls (state and the packet in flight carried)."""
    if not pyref.s2_ts_available():
        pytest.skip("oracle/_ref/libsdref_dvbs2.so (with the TS parser) not built")
    kbch = 14232 if name == "short_fields" else 43040  # short 8/9 ... normal 2/3 (BBFrameBCH::dataSize())
    frames, sent = ts_bbframes(kbch, **kw)
    want = pyref.s2_ts_extract(frames, kbch)
    got = _ts_run(capi, frames, kbch)
    assert got.shape == want.shape and np.array_equal(got, want), (name, got.shape, want.shape)
    n = len(frames)
    got2 = _ts_run(capi, frames, kbch, cuts=[0, 1, 2, 7, n // 2, n - 1, n])
    assert got2.shape == want.shape and np.array_equal(got2, want), (name, "ragged calls")
    assert len(want) > 10
    if name == "full_frames":  # sanity of the model: what comes out are the packets that went in
        sent_set = {p.tobytes() for p in sent}
        assert all(p.tobytes() in sent_set for p in want)
