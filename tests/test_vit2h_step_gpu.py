"""The path-history forward pass (k_vit2h_acs: v2h_step / v2h_group, fec_kernels.hip) at the smallest shapes that reach every lane role --
the chained-start lane, a middle lane, the tail lane with its six extra steps --, bit for bit against CCDecoder::work, and against the
decision-word kernels (k_vit2_acs / k_vit2_tb, SDHIP_VIT2_HIST=0: the independent implementation of the same trellis) on the same inputs.
The `ties` input has many equal candidates in every step: there the tie-breaking tag in the branch constants alone decides the output."""
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
    """tests/test_fec_gpu.py::_symbols (`noise`, `saturated`: the uint8 metric wrap), and `ties`: symbols next to the erasure value only."""
    stride = 2 * (F + 6)
    bits = rng.integers(0, 2, nb * F + 64).astype(np.uint8)
    coded = synth.conv_encode(bits)[: nb * 2 * F]
    if kind == "noise":
        soft = rng.integers(-127, 128, nb * 2 * F)
    elif kind == "saturated":  # full-scale symbols: exercises the uint8 metric wrap of the generic ACS kernel
        soft = (coded.astype(np.int64) * 2 - 1) * 127
        flip = rng.random(len(soft)) < 0.04
        soft = np.where(flip, -soft, soft)
    elif kind == "ties":  # {126, 127, 129} and 20 % erasures (128): branch metrics differ by 0 or 1 unit, many candidates are equal in every step
        u = rng.choice(np.array([126, 127, 129], dtype=np.int64), size=nb * 2 * F)
        u[rng.random(len(u)) < 0.2] = 128
        soft = None
    elif kind == "full_u8":  # the whole byte range: 255 never arises from soft + 127 (tests/test_soft_rails_gpu.py)
        u = rng.integers(0, 256, nb * 2 * F)
        soft = None
    else:
        raise ValueError(kind)
    if soft is not None:
        u = soft + 127
        u[u == 128] = 127
    syms = np.full(nb * stride, 128, dtype=np.uint8)
    for b in range(nb):
        syms[b * stride: b * stride + 2 * F] = u[b * 2 * F:(b + 1) * 2 * F]
    return syms


NB = 3  # chained blocks: the first has no predecessor, the others take the chained start state
# (F, SDHIP_VIT2_SEG): two 512-step segments (chained-start lane + tail lane); a middle segment added; three 1024-step segments
_CASES = [(1024, None), (1536, None), (3072, 1024)]
_KINDS = ["noise", "saturated", "ties"]
_REF = {}


def _case(orc, F, kind):
    """(symbols, the reference's bits) of one case: computed once, shared by the tests below and left unchanged."""
    key = (F, kind, orc.path)
    if key not in _REF:
        syms = _symbols(np.random.default_rng(1000 * F + _KINDS.index(kind)), F, NB, kind)
        want = orc.ccdecoder(F, syms)
        syms.setflags(write=False)
        want.setflags(write=False)
        _REF[key] = (syms, want)
    return _REF[key]


def _decode(torch, capi, F, syms):
    d_syms = _dev(torch, syms)
    d_out = torch.zeros(NB * F, dtype=torch.uint8, device="cuda")
    rc = capi.lib().sdhip_op_ccdecoder(0, F, C.c_void_p(d_syms.data_ptr()), NB, C.c_void_p(d_out.data_ptr()))
    assert rc == 0, capi.last_error()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("kind", _KINDS)
@pytest.mark.parametrize("F,seg", _CASES)
def test_history_forward_pass_bit_exact(torch_cuda, capi, orc, F, seg, kind, monkeypatch):
    """sdhip_op_ccdecoder through k_vit2h_acs / k_vit2h_tb == CCDecoder::work over three chained blocks, every bit."""
    if seg is not None:
        monkeypatch.setenv("SDHIP_VIT2_SEG", str(seg))
    monkeypatch.delenv("SDHIP_VIT2_HIST", raising=False)
    syms, want = _case(orc, F, kind)
    if kind == "ties":  # the input does what it is meant to: the reference's answer is no constant, and no symbol is far from the erasure value
        assert 0.2 < want.mean() < 0.8 and set(np.unique(syms)) == {126, 127, 128, 129}
    got = _decode(torch_cuda, capi, F, syms)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("kind", _KINDS)
@pytest.mark.parametrize("F,seg", _CASES)
def test_history_equals_decision_words(torch_cuda, capi, orc, F, seg, kind, monkeypatch):
    """The same inputs through the decision-word kernels (SDHIP_VIT2_HIST=0, read per launch): equal bits, and both the reference's."""
    if seg is not None:
        monkeypatch.setenv("SDHIP_VIT2_SEG", str(seg))
    syms, want = _case(orc, F, kind)
    monkeypatch.setenv("SDHIP_VIT2_HIST", "0")
    words = _decode(torch_cuda, capi, F, syms)
    monkeypatch.delenv("SDHIP_VIT2_HIST")
    hist = _decode(torch_cuda, capi, F, syms)
    assert np.array_equal(hist, words)
    assert np.array_equal(words, want)


def _run_stream(torch, capi, cfg, soft):
    dec = capi.FecDecoder(cfg)
    d_soft = _dev(torch, soft)
    cap = len(soft) // 4096 + 16
    d_out = torch.zeros((cap, dec.cadu_bytes), dtype=torch.uint8, device="cuda")
    n = dec.process_dev(d_soft.data_ptr(), len(soft), d_out.data_ptr(), cap)
    st = dec.stats()
    ber, state = dec.block_taps()
    out = d_out[:n].cpu().numpy()
    dec.close()
    return out, ber, state, st


def _both_settings(torch, capi, cfg, soft, monkeypatch):
    monkeypatch.delenv("SDHIP_VIT2_HIST", raising=False)
    hist = _run_stream(torch, capi, cfg, soft)
    monkeypatch.setenv("SDHIP_VIT2_HIST", "0")
    words = _run_stream(torch, capi, cfg, soft)
    monkeypatch.delenv("SDHIP_VIT2_HIST")
    (gc, gb, gs, gst), (wc, wb, ws, wst) = hist, words
    assert gc.shape == wc.shape and np.array_equal(gc, wc)
    assert np.array_equal(gb.view(np.uint32), wb.view(np.uint32)) and np.array_equal(gs, ws)
    assert np.float32(gst.viterbi_ber).view(np.uint32) == np.float32(wst.viterbi_ber).view(np.uint32)
    assert (gst.vit_respec, gst.tb_respec) == (wst.vit_respec, wst.tb_respec)
    return hist


def test_metop_stream_history_equals_decision_words(torch_cuda, capi, orc, monkeypatch):
    """A small MetOp AHRPT stream (punctured rate 3/4: the k_vit2h_acs<1, PHASE, true> instances and the speculation verdicts): CADUs,
    the Viterbi BER and the respeculation counts equal between the two settings, and the CADUs the reference's."""
    spec, cadus, plain, syms = util.metop_case(nframes=24, seed=5)
    soft = synth.soft_from_symbols(syms, spec, sigma=20, seed=2)
    cfg = capi.fec_cfg(decoder=capi.DEC_METOP_AHRPT, viterbi_ber_thresold=0.17, viterbi_outsync_after=5)
    got, _, _, st = _both_settings(torch_cuda, capi, cfg, soft, monkeypatch)
    want = orc.metop_decode(soft)
    assert len(want["cadu"]) >= 10 and got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"])


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_qpsk_stream_history_equals_decision_words(torch_cuda, capi, orc, rot, monkeypatch):
    """A small QPSK rate-1/2 stream turned by rot quarter turns (the k_vit2h_acs<0, PHASE, true> instances): as above."""
    spec, cadus, plain, syms = util.npp_case(nframes=16, seed=9)
    soft = synth.soft_from_symbols(syms, spec, sigma=30, seed=1)
    for _ in range(rot):
        s2 = soft.copy()
        s2[0::2], s2[1::2] = soft[1::2], -soft[0::2]
        soft = s2
    cfg = capi.fec_cfg(constellation="qpsk", nrzm=1, rs_i=4, rs_type=capi.RS223, rs_usecheck=1)
    got, _, _, st = _both_settings(torch_cuda, capi, cfg, soft, monkeypatch)
    want = orc.concat_decode(pyref.fec_cfg(constellation=pyref.QPSK, nrzm=1, rs_usecheck=1), soft)
    assert len(want["cadu"]) >= 6 and got.shape == want["cadu"].shape and np.array_equal(got, want["cadu"])
