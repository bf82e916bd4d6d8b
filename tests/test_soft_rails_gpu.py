"""The int8 rails at every soft-input decoder: -128 (which rotate_soft turns into -127 before anything is swapped, turned or negated, rotation.cpp:9-11;
DESIGN.md 2, "the -128 rule"), 0 at the hard-decision slicers, and 255 at the raw-symbol Viterbi op. Every other soft stream of the suite is clipped to
[-127, 127]; these streams carry -128 at every strong negative symbol and at a random share of all bytes, the way a producer that saturates to the full int8
range writes them. Everything goes through the C ABI and is held bit for bit to pyref.best(): CADUs, the per-block BER (as uint32) and lock state, the frame
and error counters. tests/test_soft_rails_on_twin_cpu.py collects the same functions against the host twin."""
import numpy as np
import pytest

from oracle import pyref
from satdump_amd import synth
from tests import test_fy3_gpu as FY
from tests import test_lrpt_gpu as LR
from tests import test_vit2h_step_gpu as V
from tests import util
from tests.test_fec_gpu import _run_dev

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


def _rails(soft, seed, p=0.05, block=8192, zeros=0.0, negative_only=False):
    """`soft` with every byte <= -110 at -128, then a random share p of all bytes at -128 (and, so that the input property below never hangs on the draw, the
    last byte of every third block). zeros: a further share of the bytes at 0. negative_only: of the random share only the bytes that are negative already --
    half of a random -128 is a full-scale sign error, which an uncoded stream or a punctured code cannot carry at 2 % of the bytes; there the rail is what
    a saturating producer makes of it, a strong negative symbol."""
    s = np.array(soft, dtype=np.int8)
    s[s <= -110] = -128
    rng = np.random.default_rng(seed)
    s[(rng.random(len(s)) < p) & ((s < 0) | (not negative_only))] = -128
    s[block - 1::3 * block] = -128
    if zeros:
        s[rng.random(len(s)) < zeros] = 0
    return s


def _assert_rails(s, block=8192, zeros=False):
    """The input is what it claims: at least 2 % of the bytes are -128, at even and odd positions, in all four byte lanes of a dword and at a block's last byte."""
    m = np.asarray(s) == -128
    assert m.mean() >= 0.02, m.mean()
    assert m[0::2].any() and m[1::2].any()
    assert all(m[k::4].any() for k in range(4))
    assert m[block - 1::block].any()
    if zeros:
        assert (np.asarray(s) == 0).mean() >= 0.02


def _need(orc, symbol):
    if not hasattr(orc.lib, symbol):
        pytest.skip("needs the compiled reference")


def _quarter_turns(soft, rot):
    for _ in range(rot):
        s2 = soft.copy()
        s2[0::2], s2[1::2] = soft[1::2], -soft[0::2]
        soft = s2
    return soft


# ---------------------------------------------------------------- ccsds_conv_concat_decoder, rate 1/2, and metop_ahrpt_decoder
_STREAMS = {}  # name -> (cfg keywords, soft, block bytes, CADUs the reference alone must deliver): built once, shared and left unchanged
_WANT = {}
_DEFAULT = {}


def _stream(name):
    if name in _STREAMS:
        return _STREAMS[name]
    junk = lambda n, seed: np.random.default_rng(seed).integers(-90, 90, n).astype(np.int8)
    tail = lambda n, seed: np.random.default_rng(seed).integers(-127, 128, n).astype(np.int8)
    if name.startswith("qpsk_rot") or name == "oqpsk":
        spec, _, _, syms = util.npp_case(nframes=12, seed=9)
        soft = _quarter_turns(synth.soft_from_symbols(syms, spec, sigma=30, seed=1), 1 if name == "oqpsk" else int(name[-1]))
        const = "oqpsk" if name == "oqpsk" else "qpsk"
        kw, block, least = dict(constellation=const, nrzm=1, rs_i=4, rs_type=pyref.RS223, rs_usecheck=1), 8192, 6
    elif name in ("bpsk", "bpsk_90"):
        # bpsk: an odd number of bytes in front, so the lock is found at shift 1; bpsk_90 (I and Q swapped, decoded at PHASE_90): a bpsk stream with every odd byte negated
        spec, _, _, syms = util.goes_case(nframes=12, seed=3)
        soft = synth.soft_from_symbols(syms, spec, sigma=30, seed=5, scale=90.0)  # strong enough to saturate: one negative symbol in four is <= -110
        if name == "bpsk_90":
            soft = soft.copy()
            soft[1::2] = -soft[1::2]
        soft = np.concatenate([junk(3001 if name == "bpsk" else 3000, 6), soft, tail(8192 + 2048, 7)])
        soft = soft[: len(soft) // 8192 * 8192]
        kw, block, least = dict(constellation=name, nrzm=1, rs_i=4, rs_type=pyref.RS223, rs_usecheck=1), 8192, 6
    elif name == "metop":
        spec, _, _, syms = util.metop_case(nframes=24, seed=5)
        soft = synth.soft_from_symbols(syms, spec, sigma=20, seed=2)
        kw, block, least = dict(decoder="metop", viterbi_ber_thresold=0.17, viterbi_outsync_after=5), 16384, 10
    else:
        raise ValueError(name)
    p = _P.get(name, 0.05)
    s = _rails(soft, seed=40 + len(name), p=p, block=block)
    s.setflags(write=False)  # shared by the tests below: they hand copies to the device
    _STREAMS[name] = (kw, s, block, least)
    return _STREAMS[name]


# the share of random -128s where the reference alone falls short of its bound at 5 % (the bound stays, the share goes down): half of the random ones are
# full-scale errors, and at one byte per symbol 5 % of them leave the reference's RS no frame it can correct (0 of 12 CADUs; 11 of 12 at 2 %)
_P = {"bpsk": 0.02, "bpsk_90": 0.02}


def _cfgs(capi, kw):
    """(capi cfg, oracle cfg or None for MetOp) of a stream's keywords"""
    kw = dict(kw)
    if kw.get("decoder") == "metop":
        kw["decoder"] = capi.DEC_METOP_AHRPT
        return capi.fec_cfg(**kw), None
    return capi.fec_cfg(**kw), pyref.fec_cfg(**dict(kw, constellation=getattr(pyref, kw["constellation"].upper())))


def _want(orc, capi, name):
    key = (name, orc.path)
    if key not in _WANT:
        kw, soft, block, least = _stream(name)
        _, oc = _cfgs(capi, kw)
        _WANT[key] = orc.metop_decode(soft) if oc is None else orc.concat_decode(oc, soft)
    return _WANT[key]


def _check_stream(name, want, run, block, least):
    got, ber, state, st = run
    assert len(want["cadu"]) >= least, (name, len(want["cadu"]))  # the reference alone stays useful on this input
    assert got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"])
    assert np.array_equal(state, want["state"])
    assert np.array_equal(ber.view(np.uint32), want["ber"].view(np.uint32))
    assert st.frames_out == len(want["cadu"])
    if "n_deframed" in want:
        assert st.frames_deframed == want["n_deframed"]
    assert list(st.rs_errors[:4]) == [int(e) for e in want["frm_err"][-1]]


def _default_run(torch, capi, name, monkeypatch):
    key = (name, capi.LIB_PATH)
    if key not in _DEFAULT:
        monkeypatch.delenv("SDHIP_VIT2_HIST", raising=False)
        monkeypatch.delenv("SDHIP_VIT2_FUSED", raising=False)
        kw, soft, _, _ = _stream(name)
        _DEFAULT[key] = _run_dev(torch, capi, _cfgs(capi, kw)[0], soft.copy())
    return _DEFAULT[key]


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_concat_qpsk_rails(torch_cuda, capi, orc, rot, monkeypatch):
    """QPSK r = 1/2 NRZ-M in all four quarter turns (k_vit2h_acs<0, PHASE, true>: V2Fetch::conv4's byte-parallel clamp): the reference delivers 9-11 of 12 CADUs."""
    name = f"qpsk_rot{rot}"
    kw, soft, block, least = _stream(name)
    _assert_rails(soft, block)
    _check_stream(name, _want(orc, capi, name), _default_run(torch_cuda, capi, name, monkeypatch), block, least)


@pytest.mark.parametrize("name", ["bpsk", "bpsk_90", "oqpsk"])
def test_concat_bpsk_family_rails(torch_cuda, capi, orc, name, monkeypatch):
    """bpsk locked at an odd shift (decode()'s `c.shift & 1` branch), bpsk_90 in three ragged calls, oqpsk a quarter turn off."""
    kw, soft, block, least = _stream(name)
    _assert_rails(soft, block)
    want = _want(orc, capi, name)
    if name == "bpsk":
        assert want["n_deframed"] > 0  # (which shift locked is the decoder's own business; the stream starts on an odd byte)
    if name == "bpsk_90":
        n = len(soft)
        monkeypatch.delenv("SDHIP_VIT2_HIST", raising=False)
        monkeypatch.delenv("SDHIP_VIT2_FUSED", raising=False)
        run = _run_dev(torch_cuda, capi, _cfgs(capi, kw)[0], soft.copy(), chunks=[0, 8192 * 3 + 17, 8192 * 11 + 5, n])
    else:
        run = _default_run(torch_cuda, capi, name, monkeypatch)
    _check_stream(name, want, run, block, least)


def test_metop_rails(torch_cuda, capi, orc, monkeypatch):
    """MetOp AHRPT (rate 3/4, k_vit2h_acs<1, PHASE, true>): at least 10 CADUs from the reference, as tests/test_vit2h_step_gpu.py requires of the clipped stream."""
    kw, soft, block, least = _stream("metop")
    _assert_rails(soft, block)
    _check_stream("metop", _want(orc, capi, "metop"), _default_run(torch_cuda, capi, "metop", monkeypatch), block, least)


@pytest.mark.parametrize("env", ["SDHIP_VIT2_FUSED", "SDHIP_VIT2_HIST"])
@pytest.mark.parametrize("name", ["qpsk_rot1", "metop"])
def test_fallback_paths_rails(torch_cuda, capi, orc, name, env, monkeypatch):
    """The same streams with the fused fetch or the path history switched off (both read per launch): k_vit2_prep's two clamp sites. Equal to the default
    run and to the reference."""
    kw, soft, block, least = _stream(name)
    dflt = _default_run(torch_cuda, capi, name, monkeypatch)
    monkeypatch.setenv(env, "0")
    run = _run_dev(torch_cuda, capi, _cfgs(capi, kw)[0], soft.copy())
    monkeypatch.delenv(env)
    assert np.array_equal(run[0], dflt[0]) and np.array_equal(run[1].view(np.uint32), dflt[1].view(np.uint32)) and np.array_equal(run[2], dflt[2])
    # the same symbols give the same speculation verdicts. (Rows k_vit2_prep gets wrong are not seen in the output where the certificates catch them: the engine
    # decodes those segments again from the soft bytes. The forward pass's respeculation count is where such a row shows -- the MetOp site's clamp, taken out,
    # is found here: 28 respeculated segments against 0. The traceback's count is its kernel's own: the same under SDHIP_VIT2_FUSED=0 only.)
    assert run[3].vit_respec == dflt[3].vit_respec
    if env == "SDHIP_VIT2_FUSED":
        assert run[3].tb_respec == dflt[3].tb_respec
    _check_stream(name, _want(orc, capi, name), run, block, least)


# ---------------------------------------------------------------- conv_rate != 1/2: punc_scatter over SymFetch
@pytest.mark.parametrize("rate,const,sigma,nrzm,gap", [(2, "qpsk", 17.0, 0, False), (4, "oqpsk", 11.7, 0, True)])
def test_punctured_rails(torch_cuda, capi, orc, rate, const, sigma, nrzm, gap):
    """rates 3/4 and 7/8 (the second with a loss of lock in the middle), the sigmas of tests/test_zz_punctured_gpu.py. A punctured code has little to spare (the
    reference delivers 0 to 2 of 8 CADUs with 2 % of all bytes at -128): the rails go to negative bytes only. At least half of the frames that can come out:
    8 without the gap, 4 with it (the reference's count on the clipped stream)."""
    soft, plain = util.punctured_case(rate, nframes=8, sigma=sigma, seed=11 + rate, nrzm=bool(nrzm), gap=gap)
    soft = _rails(soft, seed=rate, p=0.06, negative_only=True)
    _assert_rails(soft)
    want = orc.concat_decode_punc(pyref.fec_cfg(constellation=getattr(pyref, const.upper()), nrzm=nrzm, rs_usecheck=1), rate, soft)
    assert len(want["cadu"]) >= (2 if gap else 4), len(want["cadu"])
    dec = capi.FecDecoder(capi.fec_cfg(constellation=const, nrzm=nrzm, rs_i=4, rs_type=1, rs_usecheck=1, conv_rate=rate))
    cuts = [0, len(soft) // 3 // 8192 * 8192 + 777, len(soft)]
    got = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        dec.push(soft[a:b])
        got.append(dec.pull())
    got = np.concatenate(got)
    st = dec.stats()
    dec.close()
    assert got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"])
    assert st.frames_deframed == want["n_deframed"] and st.viterbi_lock == int(want["state"][-1])
    assert np.float32(st.viterbi_ber).view(np.uint32) == want["ber"][-1:].view(np.uint32)[0]
    assert list(st.rs_errors[:4]) == [int(e) for e in want["frm_err"][-1]]


# ---------------------------------------------------------------- ccsds_simple_psk_decoder: only the sign counts, the edge byte is 0
@pytest.mark.parametrize("name", ["bpsk_nrzm", "qpsk_90deg", "qpsk_diff_swap", "qpsk_delay_diff"])
def test_simple_psk_rails_and_zeros(torch_cuda, capi, orc, name):
    """hard_raw / hard_sym: -128 through the swap, the quarter turn (-(-128) is positive, as after rotate_soft's clamp) and the delay line, and 3 % of the bytes
    at 0, where `> 0` and its negation under a turn disagree with `>= 0`. The stream is uncoded: the rails go to negative bytes only, and the zeros (every other
    one a bit error, 11 % of the bytes of a codeword) are more than RS corrects, so rs_usecheck is off and every deframed frame comes out as the slicer made it
    -- each hard decision is in the compared bytes. At least 6 of the 12 frames must be deframed by the reference."""
    ck, soft, plain = util.simple_case(name, sigma=15.0, nframes=12)
    if name == "qpsk_delay_diff":
        # util's stream for this entry does not model the delay (the reference deframes nothing of it): the qpsk_diff_swap stream, arranged so that the decoder's
        # I from the symbol before (oqpsk_delay) and its I/Q exchange (qpsk_swap_iq) give the pairs back -- odd bytes = I, even bytes = the NEXT symbol's Q
        _, base, plain = util.simple_case("qpsk_diff_swap", sigma=15.0, nframes=12)
        soft = base.copy()
        soft[1::2] = base[0::2]
        soft[0:-2:2] = base[3::2]
    soft = _rails(soft, seed=len(name), p=0.06, zeros=0.03, negative_only=True)
    _assert_rails(soft, zeros=True)
    ock = dict(ck, constellation={"bpsk": pyref.BPSK, "qpsk": pyref.QPSK}[ck["constellation"]])
    want = orc.simple_decode(pyref.fec_cfg(decoder=2, rs_usecheck=0, **ock), soft)
    assert len(want["cadu"]) >= 6, len(want["cadu"])
    cfg = capi.fec_cfg(decoder=capi.DEC_SIMPLE_PSK, rs_i=4, rs_type=capi.RS223, rs_usecheck=0, **ck)
    got, _, _, st = _run_dev(torch_cuda, capi, cfg, soft)
    assert st.frames_deframed == want["n_deframed"] and st.frames_out == len(want["cadu"])
    assert list(st.rs_errors[:4]) == [int(e) for e in want["frm_err"][-1]]
    assert got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"])


# ---------------------------------------------------------------- the plugin decoders: FengYun-3 AHRPT / MPT, Meteor LRPT
def _helpers(torch):
    def to_dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return (t, t.data_ptr())

    def zeros_dev(n, dt):
        t = torch.zeros(n, dtype={np.int8: torch.int8, np.uint8: torch.uint8}[dt], device="cuda")
        return (t, t.data_ptr())

    return to_dev, (lambda d: d[0].cpu().numpy()), zeros_dev


@pytest.mark.parametrize("case", [FY.CASES[0], FY.CASES[1], FY.MPT_CASES[0]], ids=["ahrpt", "ahrpt_second_not_inverted", "mpt"])
def test_fy3_rails(torch_cuda, capi, orc, case):
    """k_fy_rails: the module's rotate_soft over the read, then each rail's own (and the second rail's complement, which makes a -128 of every 127)."""
    mpt, inv2 = case.get("mpt", False), case.get("invert_second", True)
    _need(orc, "sdref_fy3_mpt_decode" if mpt else "sdref_fy3_decode")
    soft, plain = synth.fy3_ahrpt_soft(**case)
    soft = _rails(soft, seed=3 + int(inv2), p=0.02, block=16384)  # (at 5 % the reference delivers 3 and 9 of 24 CADUs, at 2 % 21 to 23: each rail is a rate-3/4 code)
    _assert_rails(soft, 16384)
    want = orc.fy3_mpt_decode(soft) if mpt else orc.fy3_decode(soft, invert_second=inv2)
    assert len(want["cadu"]) >= case["nframes"] // 2, len(want["cadu"])
    got, ber, state, st = FY.run_engine(capi, *_helpers(torch_cuda), soft, invert_second=inv2, mpt=mpt)
    assert np.array_equal(state, want["state"])
    assert np.array_equal(ber.view(np.uint32), want["ber"].view(np.uint32))
    assert got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"])
    assert list(st.rs_errors[:4]) == list(want["frm_err"][-1]) and st.frames_out == len(want["cadu"])
    assert st.viterbi_lock == want["state"][-1, 0] and st.viterbi2_lock == want["state"][-1, 1]


@pytest.mark.parametrize("kw", [dict(nframes=10, turn=1, swap=True), dict(nframes=14, diff=True, sigma=25.0)], ids=["turn1_swap", "diff"])
def test_lrpt_rails(torch_cuda, capi, orc, kw):
    """k_lrpt_gather: the clamp in front of the I/Q swap and the quarter turns the correlator asks for."""
    _need(orc, "sdref_lrpt_decode")
    soft, plain = LR.lrpt_soft(**kw)
    soft = _rails(soft, seed=kw["nframes"], block=16384)
    _assert_rails(soft, 16384)
    diff = kw.get("diff", False)
    want = orc.lrpt_decode(soft, diff)["cadu"]
    assert len(want) >= kw["nframes"] // 2, len(want)
    got, st = LR.run_engine(capi, *_helpers(torch_cuda), soft, diff)
    # (the module's extra iterations on a stale buffer at the end of a file are not reproduced: tests/test_lrpt_gpu.py::check_decoder)
    assert len(got) <= len(want) <= len(got) + 2, (len(got), len(want))
    assert np.array_equal(got, want[: len(got)])
    assert st.frames_out == len(got) and st.soft_in == len(soft)


def test_lrpt_m2x_rails(capi, orc):
    """m2x_mode + interleaved on a stream a quarter turn off, where the SECOND reader (the file's 8192-byte chunks through rotate_soft at PHASE_90) is the one
    whose Viterbi locks: m2x_clamp in both readers. The transmitted stream gets its rails after the turn, markers included."""
    from tests.test_lrpt_m2x_reference_cpu import LEAD
    _need(orc, "sdref_lrpt_m2x_decode")
    nframes = 40
    soft, plain = LR.lrpt_soft(nframes, seed=7, diff=True, sigma=18.0)
    pre = np.random.default_rng(8).integers(-60, 60, LEAD).astype(np.int8)
    tx = synth.m2x_interleave(np.concatenate([pre, soft]), marker_amp=-90, seed=7)
    t = tx[: len(tx) // 2 * 2].reshape(-1, 2).astype(np.int16)
    tx = _rails(np.stack([-t[:, 1], t[:, 0]], axis=1).reshape(-1).clip(-127, 127).astype(np.int8), seed=9, p=0.03)
    _assert_rails(tx)
    want = orc.lrpt_m2x_decode(tx, diff_decode=True, interleaved=True, reader_returns=1)
    assert len(want["cadu"]) >= nframes - 12, len(want["cadu"])
    assert (want["which"] == 2).any()
    got, ber, state, st = LR.m2x_run_hip(capi, tx)
    assert got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"])
    assert len(state) == want["iterations"] and np.array_equal(state, want["state"])
    assert np.array_equal(ber.view(np.uint32), want["ber"].view(np.uint32))
    assert st.frames_out == len(want["cadu"])


# ---------------------------------------------------------------- sdhip_op_ccdecoder: raw unsigned symbols, the whole byte range
@pytest.mark.parametrize("hist", [None, "0"], ids=["history", "decision_words"])
@pytest.mark.parametrize("F", [1024, 1536])
def test_ccdecoder_full_u8(torch_cuda, capi, orc, F, hist, monkeypatch):
    """Symbols drawn from 0 .. 255: 255 never arises from soft + 127 and 0 only from -127; three chained blocks against CCDecoder::work."""
    syms = V._symbols(np.random.default_rng(7 * F), F, V.NB, "full_u8")
    assert (syms == 255).any() and (syms == 0).any() and (syms == 128).any()
    want = orc.ccdecoder(F, syms)
    if hist is None:
        monkeypatch.delenv("SDHIP_VIT2_HIST", raising=False)
    else:
        monkeypatch.setenv("SDHIP_VIT2_HIST", hist)
    got = V._decode(torch_cuda, capi, F, syms)
    assert got.shape == want.shape and np.array_equal(got, want)
