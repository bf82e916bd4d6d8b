"""What a handle finds in its blocks. Every device and pinned block of the library comes from dev_alloc / pin_alloc (satdump_amd/csrc/fec_engine.hip), and
the product runs with the block pool on (bench.py's multi-rank steps: a fresh demodulator and decoder per step, their blocks recycled with the previous owner's
contents) and with several handles alive in one process (the plugin's pipeline). Three legs, every comparison an equality of bytes, float bit patterns and statistics:

  A  filled blocks: under SDHIP_ALLOC_FILL = 255 (NaN, -1) and 127 (3.4e38, +127) every family's result is still what its own test demands of it (oracle or golden
     file; the existing helpers and test bodies are called, not copied), and pool_stats().filled has advanced;
  B  recycled blocks: pool on, stream A through handle 1, then stream B (another seed, the same length, the same call sizes) through handle 2 == stream B through a
     fresh handle with the pool off; blocks must have been parked in between and recycled by handle 2, or the run has tested nothing and fails; a handle that grows
     in mid-run; pool_enable(False) / pool_trim();
  C  two live handles of different configurations, their calls alternated A1 B1 A2 B2 A3 B3 over ragged slices, each equal to its solo run; once more with the
     profiler on.

The legs complement each other: an element that NEITHER stream writes holds in a recycled block what it held in the fresh one, so leg B cannot see it (tried on the
twin: k_compact8 or k_rs_slots skipping its last element passes leg B and fails leg A); state a kernel assumes cleared and output written in part is leg B's.

Every test leaves the process as it found it (pool off, fill unset, nothing parked). tests/test_block_contents_on_twin_cpu.py collects the same functions against
the host twin."""
import contextlib
import ctypes as C
import os
import struct

import numpy as np
import pytest

from oracle import pyref
from satdump_amd import synth
from tests import dvbs2_util, util
from tests import test_aos_gpu as AOS
from tests import test_ccsds_ldpc_gpu as L
from tests import test_demod_gpu as D
from tests import test_dvbs2_gpu as G
from tests import test_fec_gpu as F
from tests import test_fsk_gpu as K
from tests import test_fy3_gpu as FY
from tests import test_lrpt_gpu as LR
from tests import test_ndsp_gpu as N
from tests import test_zz_punctured_gpu as Z

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


@pytest.fixture(scope="module")
def orc():
    return pyref.best()


@pytest.fixture(scope="module")
def mem():
    from satdump_amd import dvbs2
    return dvbs2.TorchMem


class Ctx:
    """what a family needs to run: the torch stand-in, the binding, the oracle, the DVB-S2 mirror's memory adapter, and the (to_dev, to_host, zeros_dev) trio"""

    def __init__(self, torch, capi, orc, mem):
        self.torch, self.capi, self.orc, self.mem = torch, capi, orc, mem

    def to_dev(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return (t, t.data_ptr())

    def zeros_dev(self, n, dt):
        t = self.torch.zeros(n, dtype=getattr(self.torch, np.dtype(dt).name), device="cuda")
        return (t, t.data_ptr())

    @staticmethod
    def to_host(d):
        return d[0].cpu().numpy()

    @property
    def trio(self):
        return self.to_dev, self.to_host, self.zeros_dev


@pytest.fixture()
def ctx(torch_cuda, capi, orc, mem):
    return Ctx(torch_cuda, capi, orc, mem)


def _nref():
    if not pyref.NdspRef.available():
        pytest.skip("oracle/_ref/libsdref_ndsp.so not built")
    return pyref.NdspRef()


def _need_ref(symbol):
    if not (pyref.ref_available() and hasattr(pyref.ref().lib, symbol)):
        pytest.skip("needs the compiled reference")


@contextlib.contextmanager
def _clean_state(capi):
    """the process state every test starts from and restores: pool off, fill unset, nothing parked"""
    old = os.environ.pop("SDHIP_ALLOC_FILL", None)
    capi.pool_enable(False)
    try:
        yield
    finally:
        os.environ.pop("SDHIP_ALLOC_FILL", None)
        if old is not None:
            os.environ["SDHIP_ALLOC_FILL"] = old
        capi.pool_enable(False)
        capi.prof_enable(False)
        st = capi.pool_stats()
        assert (st.dev_parked, st.pin_parked, st.dev_parked_bytes, st.pin_parked_bytes) == (0, 0, 0, 0)


def _flat(v):
    """a result as something == compares bit for bit: arrays as (dtype, shape, bytes), floats as their bits, ctypes structures field by field"""
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, np.ascontiguousarray(v).tobytes())
    if isinstance(v, C.Structure):
        return tuple((n, _flat(getattr(v, n))) for n, _ in v._fields_)
    if isinstance(v, C.Array):
        return tuple(_flat(e) for e in v)
    if isinstance(v, dict):
        return tuple((k, _flat(v[k])) for k in sorted(v))
    if isinstance(v, (tuple, list)):
        return tuple(_flat(e) for e in v)
    if isinstance(v, (float, np.floating)):
        return struct.pack("<d", float(v))
    return v


def _assert_same(got, want, what):
    g, w = _flat(got), _flat(want)
    assert len(g) == len(w), what
    for k, (a, b) in enumerate(zip(g, w)):
        assert a == b, f"{what}: part {k} of the result differs"


def _ragged(n, unit=1):
    """three ragged calls over n items (A1 A2 A3)"""
    return [0, (n // 3 + 17) // unit * unit + (777 if unit > 1 else 0), 2 * n // 3 + 5, n]


# ================================================================ the families: one handle each, open -> step(0), step(1), ... -> close() = the result
class FecRun:
    """FecDecoder (any `decoder`) over a stream resident on the device, or through push / pull"""
    pinned = False

    def __init__(self, ctx, cfg, soft, cuts=None, host=False):
        self.ctx, self.soft, self.host = ctx, np.ascontiguousarray(soft), host
        self.cuts = cuts or [0, len(soft)]
        self.dec = ctx.capi.FecDecoder(cfg)
        self.d_soft = None if host else ctx.to_dev(self.soft)
        self.out = []

    def step(self, i):
        a, b = self.cuts[i], self.cuts[i + 1]
        if self.host:
            self.dec.push(self.soft[a:b])
            self.out.append((self.dec.pull(),))
            return
        cap = (b - a) // 1024 + 16
        d_out = self.ctx.zeros_dev(cap * self.dec.cadu_bytes, np.uint8)
        n = self.dec.process_dev(self.d_soft[1] + a, b - a, d_out[1], cap)
        self.out.append((self.ctx.to_host(d_out)[: n * self.dec.cadu_bytes].copy(),) + tuple(self.dec.block_taps()))

    def close(self):
        st = self.dec.stats()
        getattr(self, "before_destroy", lambda: None)()  # (test_a_handle_that_grows looks at the pool here: the handle has done all its work and still owns its buffers)
        self.dec.close()
        return tuple(np.concatenate([o[k] for o in self.out]) for k in range(len(self.out[0]))) + (st,)


class DemodRun:
    """PskDemod / FskDemod: samples in, soft bytes and float symbols out (the whole symbol buffer of every call is compared, written or not)"""

    def __init__(self, ctx, dem, raw, fmt, cuts=None, host=False):
        self.ctx, self.dem, self.fmt, self.host = ctx, dem, fmt, host
        self.raw = np.ascontiguousarray(raw)  # two scalars per sample
        self.n = self.raw.size // 2
        self.cuts = cuts or [0, self.n]
        self.d_x = None if host else ctx.to_dev(self.raw)
        self.out = []

    def step(self, i):
        a, b = self.cuts[i], self.cuts[i + 1]
        n = b - a
        if self.host:
            self.dem.push(self.raw[2 * a: 2 * b], self.fmt)
            return
        d_soft, d_syms = self.ctx.zeros_dev(2 * n + 64, np.int8), self.ctx.zeros_dev(2 * (n + 64), np.float32)
        ns = self.dem.process_dev(self.d_x[1] + 2 * a * self.raw.itemsize, n, self.fmt, d_soft[1], 2 * n + 64, d_syms[1], n + 64)
        self.out.append((self.ctx.to_host(d_soft)[:ns].copy(), self.ctx.to_host(d_syms).view(np.uint32).copy()))

    def close(self):
        if self.host:
            self.dem.flush()
            self.out.append((self.dem.pull(), np.zeros(0, np.uint32)))
        st = self.dem.stats()
        getattr(self, "before_destroy", lambda: None)()  # (test_a_handle_that_grows looks at the pool here: the handle has done all its work and still owns its buffers)
        self.dem.close()
        return (np.concatenate([o[0] for o in self.out]), np.concatenate([o[1] for o in self.out]), st)


class LrptRun:
    def __init__(self, ctx, soft, diff, cuts=None, host=False):
        self.ctx, self.soft, self.host, self.lib = ctx, np.ascontiguousarray(soft), host, ctx.capi.lib()
        self.cuts = cuts or [0, len(soft)]
        cfg = ctx.capi.LrptCfg()
        self.lib.sdhip_lrpt_cfg_default(C.byref(cfg))
        cfg.diff_decode = int(diff)
        self.h = self.lib.sdhip_lrpt_create(C.byref(cfg))
        assert self.h, ctx.capi.last_error()
        self.out = []

    def step(self, i):
        a, b = self.cuts[i], self.cuts[i + 1]
        cap = (b - a) // 16384 + 4
        if self.host:
            blk = np.ascontiguousarray(self.soft[a:b])
            assert self.lib.sdhip_lrpt_push(self.h, blk.ctypes.data_as(C.c_void_p), len(blk)) == 0, self.ctx.capi.last_error()
            buf = np.zeros((cap, 1024), dtype=np.uint8)
            k = self.lib.sdhip_lrpt_pull(self.h, buf.ctypes.data_as(C.c_void_p), cap)
            self.out.append(buf[:k].reshape(-1).copy())
            return
        d_in, d_out = self.ctx.to_dev(self.soft[a:b]), self.ctx.zeros_dev(cap * 1024, np.uint8)
        n = self.lib.sdhip_lrpt_process_dev(self.h, C.c_void_p(d_in[1]), b - a, C.c_void_p(d_out[1]), cap)
        assert n >= 0, self.ctx.capi.last_error()
        self.out.append(self.ctx.to_host(d_out)[: n * 1024].copy())

    def close(self):
        st = self.ctx.capi.LrptStats()
        self.lib.sdhip_lrpt_get_stats(self.h, C.byref(st))
        getattr(self, "before_destroy", lambda: None)()  # (test_a_handle_that_grows looks at the pool here: the handle has done all its work and still owns its buffers)
        self.lib.sdhip_lrpt_destroy(self.h)
        return (np.concatenate(self.out), st)


class CcsdsRun:
    def __init__(self, ctx, cfg, soft, cuts=None, host=False):
        self.ctx, self.soft, self.host = ctx, np.array(soft, copy=True), host
        self.cuts = cuts or [0, len(soft)]
        self.dec = ctx.capi.CcsdsLdpc(cfg)
        self.d_x = None if host else ctx.to_dev(self.soft)
        self.out = []

    def step(self, i):
        a, b = self.cuts[i], self.cuts[i + 1]
        cap = (b - a) // L.F + 4
        if self.host:
            self.dec.push(self.soft[a:b])
            self.out.append((self.dec.pull(cap).reshape(-1), self.dec.descs()))
            return
        d_out = self.ctx.zeros_dev(cap * self.dec.frame_bytes, np.uint8)
        k = self.dec.process_dev(self.d_x[1] + a, b - a, d_out[1], cap)
        self.out.append((self.ctx.to_host(d_out)[: k * self.dec.frame_bytes].copy(), self.dec.descs()))

    def close(self):
        st = self.dec.stats()
        getattr(self, "before_destroy", lambda: None)()  # (test_a_handle_that_grows looks at the pool here: the handle has done all its work and still owns its buffers)
        self.dec.close()
        return (np.concatenate([o[0] for o in self.out]), np.concatenate([o[1] for o in self.out]), st)


class S2FecRun:
    """LdpcDecoder + BchDecoder on frames resident on the device, the tail of DVBS2DemodModule::process_s2: decode, repack, BCH, descramble; a step = some frames"""
    TRIALS = 12

    def __init__(self, ctx, fs, rate, seed, sigma, cuts):
        self.ctx, self.cuts = ctx, cuts
        self.ldpc = ctx.capi.LdpcDecoder(framesize=fs, rate=rate, batch=1)
        self.bch = ctx.capi.BchDecoder(framesize=fs, rate=rate)
        n, k = self.ldpc.info.code_len, self.ldpc.info.data_len
        assert self.bch.nbch == k
        self.n, self.k = n, k
        self.soft = _s2_soft(fs, ctx.capi.S2_RATES[rate], cuts[-1], k, seed, sigma)
        self.out = []

    def step(self, i):
        a, b = self.cuts[i], self.cuts[i + 1]
        nf, ctx = b - a, self.ctx
        d_soft = ctx.to_dev(self.soft[a:b].copy())
        d_tr, d_corr, d_pack = ctx.zeros_dev(nf, np.int32), ctx.zeros_dev(nf, np.int32), ctx.zeros_dev(nf * (self.k // 8), np.uint8)
        self.ldpc.decode_dev(d_soft[1], nf, self.TRIALS, d_tr[1])
        self.bch.pack_dev(d_soft[1], self.n, nf, d_pack[1], self.k // 8)
        self.bch.decode_dev(d_pack[1], nf, self.k // 8, d_corr[1])
        self.bch.descramble_dev(d_pack[1], nf, self.k // 8)
        self.out.append(tuple(ctx.to_host(d).copy() for d in (d_soft, d_tr, d_pack, d_corr)))

    def close(self):
        getattr(self, "before_destroy", lambda: None)()  # (test_a_handle_that_grows looks at the pool here: the handle has done all its work and still owns its buffers)
        self.ldpc.close()
        self.bch.close()
        return tuple(np.concatenate([o[k].reshape(-1) for o in self.out]) for k in range(4))


_S2_SOFT = {}


def _s2_soft(fs, rc, nframes, k, seed, sigma):
    key = (fs, rc, nframes, seed, sigma)
    if key not in _S2_SOFT:
        rng = np.random.default_rng(seed)
        bits = dvbs2_util.encode(fs, rc, rng.integers(0, 2, (nframes, k), dtype=np.uint8))
        s = np.clip(np.rint(np.where(bits > 0, -1.0, 1.0) * 20 + rng.standard_normal(bits.shape) * sigma), -127, 127).astype(np.int8)
        s.setflags(write=False)
        _S2_SOFT[key] = s
    return _S2_SOFT[key]


class Dvbs2Run:
    """the DVB-S2 demodulator handle (satdump_amd.dvbs2.DVBS2Demod over sdhip_dvbs2_demod_*): baseband in, BBFRAMEs out, default (parallel) schedules"""

    def __init__(self, ctx, modcod, short, bbx, cuts=None):
        from satdump_amd import dvbs2
        G._dvbs2_ref_lib()
        front = pyref.S2FrontRef()
        params = {"samplerate": 2e6, "symbolrate": 1e6, "rrc_alpha": 0.2, "pll_bw": 0.002, "modcod": modcod, "shortframes": bool(short), "freq_prop_factor": 0.0, "ldpc_trials": 25}
        self.dem = dvbs2.DVBS2Demod(params, front.lut(modcod, short), pyref.s2_lut_phase_ref(modcod, short), mem=ctx.mem(), capi=ctx.capi)
        self.bbx, self.cuts, self.out = bbx, cuts or [0, len(bbx)], []
        self.acq = str(3 * (pyref.S2FrontRef().cfg(modcod, short, 0)["slots"] + 1) * 90)  # three frames of serial acquisition, as tests/test_dvbs2_gpu.py sets it

    def step(self, i):
        old = os.environ.get("SDHIP_S2PLL_ACQ")
        os.environ["SDHIP_S2PLL_ACQ"] = self.acq
        try:
            self.out.append(self.dem.process(self.bbx[self.cuts[i]: self.cuts[i + 1]]))
        finally:
            os.environ.pop("SDHIP_S2PLL_ACQ")
            if old is not None:
                os.environ["SDHIP_S2PLL_ACQ"] = old

    def close(self):
        st = dict(self.dem.stats)
        getattr(self, "before_destroy", lambda: None)()  # (test_a_handle_that_grows looks at the pool here: the handle has done all its work and still owns its buffers)
        self.dem.close()
        return (np.concatenate(self.out), st)


class NdspRun:
    """the ndsp PSK demodulator hier handle on the device path"""

    def __init__(self, ctx, x, cuts=None, **kw):
        self.ctx, self.lib, self.x = ctx, ctx.capi.lib(), x
        self.cuts = cuts or [0, len(x)]
        c = ctx.capi.NdspPskCfg()
        self.lib.sdhip_ndsp_psk_cfg_default(C.byref(c))
        for k, v in kw.items():
            setattr(c, k, v)
        self.h = self.lib.sdhip_ndsp_psk_demod_create(C.byref(c))
        assert self.h, ctx.capi.last_error()
        self.d_x = ctx.to_dev(x.view(np.float32))
        self.out = []

    def step(self, i):
        a, b = self.cuts[i], self.cuts[i + 1]
        n = b - a
        d_y = self.ctx.zeros_dev(2 * (n + 64), np.float32)
        ns = self.lib.sdhip_ndsp_psk_demod_work_dev(self.h, C.c_void_p(self.d_x[1] + 8 * a), n, C.c_void_p(d_y[1]), n + 64)
        assert ns >= 0, self.ctx.capi.last_error()
        self.out.append(self.ctx.to_host(d_y)[: 2 * ns].view(np.uint32).copy())

    def close(self):
        st = self.ctx.capi.DemodStats()
        self.lib.sdhip_ndsp_psk_demod_get_stats(self.h, C.byref(st))
        getattr(self, "before_destroy", lambda: None)()  # (test_a_handle_that_grows looks at the pool here: the handle has done all its work and still owns its buffers)
        self.lib.sdhip_ndsp_psk_demod_destroy(self.h)
        return (np.concatenate(self.out), st)


class NdspBlockRun:
    """one member block as a handle of its own (satdump_amd.ndsp.SingleBlock, host buffers in and out)"""

    def __init__(self, ctx, block_id, cfg, x, cuts=None):
        from satdump_amd import ndsp
        self.blk = ndsp.SingleBlock(block_id, exact=False, capi_mod=ctx.capi)
        for k, v in cfg.items():
            assert self.blk.set_cfg(k, v) == ndsp.RES_OK
        self.x, self.cuts, self.out = x, cuts or [0, len(x)], []

    def step(self, i):
        self.out.append(self.blk.work(self.x[self.cuts[i]: self.cuts[i + 1]]).view(np.uint32))

    def close(self):
        st = self.blk.stats()
        getattr(self, "before_destroy", lambda: None)()  # (test_a_handle_that_grows looks at the pool here: the handle has done all its work and still owns its buffers)
        self.blk.stop()
        return (np.concatenate(self.out), st)


def _solo(opener):
    h = opener()
    for i in range(len(h.cuts) - 1):
        h.step(i)
    return h.close()


# ---------------------------------------------------------------- the streams: built once, shared, left unchanged. which = "B" (the stream compared) or "A" (another seed)
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def _psk_x(name, which):
    """(demod keywords, baseband) of tests/test_demod_gpu.py's GOES (24 frames, BPSK) / NPP (40 frames, QPSK, 2 samples per symbol) / MetOp (40 frames, QPSK, 2.57 samples
    per symbol) case; A: the same case from another seed"""
    def make():
        if which == "B":
            _, _, x, _, kw, _, _ = D._case(name)
            return kw, x
        spec, _, _, syms = {"goes": lambda: util.goes_case(nframes=24, seed=7), "npp": lambda: util.npp_case(nframes=40, seed=11), "metop": lambda: util.metop_case(nframes=40, seed=8)}[name]()
        return _psk_x(name, "B")[0], synth.modulate(syms, spec)[0]
    return _cached(("psk", name, which), make)


def _fec_soft(name, which):
    """(cfg keywords, soft stream) of the decoder families"""
    def make():
        s = 0 if which == "B" else 10
        if name == "concat":  # tests/test_fec_gpu.py::test_concat_decoder_bpsk at sigma 30, 16 frames
            spec, _, _, syms = util.goes_case(nframes=16, seed=3 + s)
            return dict(constellation="bpsk", nrzm=1, rs_i=4, rs_type=1, rs_usecheck=1), synth.soft_from_symbols(syms, spec, sigma=30, seed=30 + s)
        if name == "metop":  # ::test_metop_decoder at sigma 50, 12 frames
            spec, _, _, syms = util.metop_case(nframes=12, seed=5 + s)
            return dict(decoder=1, viterbi_ber_thresold=0.17, viterbi_outsync_after=5), synth.soft_from_symbols(syms, spec, sigma=50, seed=2 + s)
        if name == "punctured":  # tests/test_zz_punctured_gpu.py: rate 3/4, QPSK
            soft, _ = util.punctured_case(2, nframes=8, sigma=17.0, seed=13 + s)
            return dict(constellation="qpsk", nrzm=0, rs_i=4, rs_type=1, rs_usecheck=1, conv_rate=2), soft
        if name == "simple":
            ck, soft, _ = util.simple_case("qpsk_diff_swap", sigma=15.0, nframes=12, seed=5 + s)
            return dict(decoder=2, rs_i=4, rs_type=1, rs_usecheck=1, **ck), soft
        if name in ("fy3", "fy3_mpt"):
            soft, _ = synth.fy3_ahrpt_soft(nframes=24, seed=3 + s, mpt=name == "fy3_mpt")
            return dict(decoder=4 if name == "fy3_mpt" else 3, viterbi_ber_thresold=0.17, viterbi_outsync_after=5, invert_second_viterbi=1), soft
        if name == "tail_rs239":  # a tests/test_fec_gpu.py::_TAIL_CASES entry: QPSK, I = 5, RS(255,239)
            return None, F._tail_case("qpsk_i5_rs239")[0]
        raise ValueError(name)
    return _cached(("fec", name, which), make)


def _fec_open(ctx, name, which, cuts=3, host=False):
    kw, soft = _fec_soft(name, which)
    cfg = F._tail_cfg(ctx.capi, "qpsk_i5_rs239", 1) if kw is None else ctx.capi.fec_cfg(**kw)
    return FecRun(ctx, cfg, soft, _ragged(len(soft), 8192) if cuts == 3 else cuts, host)


def _psk_open(ctx, name, which, exact, cuts=3, host=False):
    kw, x = _psk_x(name, which)
    dem = ctx.capi.PskDemod(ctx.capi.demod_cfg(**kw, exact=int(exact), chunk_len=0 if exact else 8192))
    return DemodRun(ctx, dem, x.view(np.float32), ctx.capi.FMT_CF32, _ragged(len(x)) if cuts == 3 else cuts, host)


def _fsk_open(ctx, name, which, exact=False, cuts=3, host=False):
    g = K._golden(name)
    cs16 = np.asarray(g["cs16"])
    if which == "A":  # the fixture's samples in reverse order: another signal of the same length
        cs16 = np.ascontiguousarray(cs16.reshape(-1, 2)[::-1]).reshape(-1)
    dem = K._handle(ctx.capi, g, exact=int(exact), chunk_len=0 if exact else K.CHUNK)
    return DemodRun(ctx, dem, cs16, ctx.capi.FMT_CS16, _ragged(len(cs16) // 2) if cuts == 3 else cuts, host)


def _lrpt_open(ctx, which, cuts=3, host=False):
    kw = dict(LR.CASES[0], seed=3 if which == "B" else 4)
    soft = _cached(("lrpt", which), lambda: LR.lrpt_soft(**kw)[0])
    return LrptRun(ctx, soft, False, _ragged(len(soft)) if cuts == 3 else cuts, host)


def _ccsds_open(ctx, name, which, cuts=3, host=False):
    g = L._golden(name)
    soft = np.asarray(g["soft"])[: 10 * L.F]  # (ten frames of the fixture: a result to compare with itself, and the twin takes seconds per frame)
    if which == "A":  # the same frames three places on: other bytes at every position, the same number of frames in every call (the deframer's buffers are sized by it)
        soft = np.roll(soft, 3 * L.F)
    return CcsdsRun(ctx, L._cfg(ctx.capi, g), soft, _ragged(len(soft)) if cuts == 3 else cuts, host)


def _s2fec_open(ctx, fs, rate, which):
    sigma = {(1, "1/2"): 16.0, (0, "2/3"): 13.0}[(fs, rate)]
    return S2FecRun(ctx, fs, rate, seed=(5 if which == "B" else 6) + fs, sigma=sigma, cuts=[0, 1, 3, 4])


def _dvbs2_open(ctx, modcod, short, which, nfr=6):
    G._dvbs2_ref_lib()
    bbx = _cached(("dvbs2", modcod, short, which, nfr), lambda: G._s2_baseband(modcod, short, nfr, 10.0, seed=3 if which == "B" else 4)[0])
    return Dvbs2Run(ctx, modcod, short, bbx, _ragged(len(bbx)))


def _ndsp_x(which, n_sym=120000):
    return _cached(("ndsp", which, n_sym), lambda: N._signal("qpsk", n_sym, 6e6, 2e6, esn0=12.0, seed=5 if which == "B" else 6))


def _ndsp_open(ctx, which):
    x = _ndsp_x(which)
    return NdspRun(ctx, x, _ragged(len(x)), constellation=ctx.capi.QPSK, samplerate=6e6, symbolrate=2e6, chunk_len=8192)


def _costas_fast_open(ctx, which):
    x = _cached(("cf", which), lambda: np.ascontiguousarray(_ndsp_x(which, 40000)[::3]))
    return NdspBlockRun(ctx, "costas_fast_cc", {"order": 4, "loop_bw": 0.004}, x, _ragged(len(x)))


# ================================================================ Leg A: filled blocks
def _a_psk(ctx, case):
    D.test_exact_mode_bit_identical(ctx.torch, ctx.capi, ctx.orc, case)
    D.test_chunked_mode_symbols_and_cadus(ctx.torch, ctx.capi, ctx.orc, case)


def _a_ndsp_qpsk(ctx):
    N.test_ndsp_psk_demod_chunk_parallel(ctx.torch, ctx.capi, _nref(), "qpsk")


def _a_s2fec(ctx, fs, rate):
    ref = G._ref(False)
    G.run_case(ctx.capi, ref, fs, rate, 2, 20, G.SIGMA[rate] * (1.0 if fs == 0 else 0.9), 12)
    G.bch_case(ctx.capi, ref, fs, rate, [0, 1, 5, 12, 13, 40])


def _a_lrpt(ctx):
    _need_ref("sdref_lrpt_decode")
    LR.check_decoder(ctx.capi, *ctx.trio, LR.CASES[0])


def _a_fy3(ctx, case):
    _need_ref("sdref_fy3_mpt_decode" if case.get("mpt") else "sdref_fy3_decode")
    FY.check_decoder(ctx.capi, *ctx.trio, case)


def _a_aos(ctx):
    if not pyref.AosRef.available():
        pytest.skip("oracle/_ref/libsdref_aos.so not built")
    AOS.check_demux(ctx.capi, ctx.to_dev, ctx.to_host, ctx.zeros_dev, AOS.CASES[0])


def _a_ccsds_unit(ctx):
    L.test_unit_decode_bit_exact(ctx.torch, ctx.capi, 10)


def _a_fsk(ctx, case):
    K.test_exact_mode_bit_identical(ctx.torch, ctx.capi, case)
    K.test_chunk_parallel_mode(ctx.torch, ctx.capi, case)


def _a_bb_to_soft(ctx):
    """sdhip_s2_bb_to_soft_dev keeps its tables and scratch rows for the life of the process (S2DemapCache): a run draws a block only where it needs a larger one than
    any run before it. More frames than any other caller hands over (four), and one more under the second fill, so that each run's scratch rows are new and filled."""
    G.check_bb_to_soft(ctx.capi, ctx.to_dev, ctx.to_host, ctx.zeros_dev, *G.BB2SOFT[3], nframes=5 + (os.environ["SDHIP_ALLOC_FILL"] == "127"))


def _a_pll_parallel(ctx):
    """sdhip_s2_pll_frames_dev keeps its last runner while configuration and table stay the same: an empty call with another configuration first, so that the case
    builds its runner anew, from filled blocks"""
    G._dvbs2_ref_lib()
    st = np.zeros(2, dtype=np.float32)
    lut = pyref.s2_lut_phase_ref(4, 1)
    rc = ctx.capi.lib().sdhip_s2_pll_frames_dev(0, 4, 1, 0, 0.002, None, None, 8190, 0, lut.ctypes.data_as(C.c_void_p), 256, st.ctypes.data_as(C.c_void_p), 2, None)
    assert rc >= 0, ctx.capi.last_error()
    G.check_pll_parallel(ctx.capi, ctx.to_dev, ctx.to_host, ctx.zeros_dev, 12, 1, 9.0, 16, 0)


FILLED = {
    "psk_goes": lambda c: _a_psk(c, "goes"),
    "psk_npp": lambda c: _a_psk(c, "npp"),
    "psk_metop_host": lambda c: D.test_host_push_pull_path(c.torch, c.capi, c.orc),  # (QPSK without the float symbols: k_compact8 writes the soft bytes)
    "concat_bpsk": lambda c: F.test_concat_decoder_bpsk(c.torch, c.capi, c.orc, 30, 1),
    "punctured": lambda c: Z.test_punctured_concat_decoder(c.torch, c.capi, c.orc, 2, "qpsk", pyref.QPSK, 20.0, 0, False),
    "metop": lambda c: F.test_metop_decoder(c.torch, c.capi, c.orc, 50),
    "simple_psk": lambda c: F.test_simple_psk_decoder(c.torch, c.capi, c.orc, "qpsk_diff_swap", 15.0, 1),
    "lrpt": _a_lrpt,
    "lrpt_m2x": lambda c: LR.test_lrpt_m2x_interleaved(c.capi, *LR.M2X_CASES[0]),
    "fy3_ahrpt": lambda c: _a_fy3(c, FY.CASES[0]),
    "fy3_mpt": lambda c: _a_fy3(c, FY.MPT_CASES[0]),
    "aos_demux": _a_aos,
    "fsk_a": lambda c: _a_fsk(c, "fsk_a"),
    "sdpsk_c": lambda c: _a_fsk(c, "sdpsk_c"),
    "ndsp_qpsk": _a_ndsp_qpsk,
    "ndsp_costas_fast": lambda c: N.check_costas_fast_chunk_parallel(c.capi, _nref()),
    "ndsp_mm_fast": lambda c: N.check_mm_fast_chunk_parallel(c.capi, _nref()),
    "ndsp_agc_fast": lambda c: N.check_single_block_handles(c.capi, _nref(), *N.SINGLE[2]),
    "s2_ldpc_bch_short_1_2": lambda c: _a_s2fec(c, 1, "1/2"),
    "s2_ldpc_bch_normal_2_3": lambda c: _a_s2fec(c, 0, "2/3"),
    "s2_bb_to_soft": _a_bb_to_soft,
    "s2_pll_parallel": _a_pll_parallel,
    "s2_engine_parallel": lambda c: G.check_dvbs2_engine(c.capi, c.mem, modcod=13, short=0, nfr=10, esn0_db=10.0, acq=2 * 21690),
    "s2_ts": lambda c: G.test_s2_ts_extractor(c.capi, *G.TS_CASES[0]),
    "ccsds_ldpc_unit": _a_ccsds_unit,
    "ccsds_ldpc_stream": lambda c: L.test_stream_three_calls(c.torch, c.capi, "r78_qpsk_direct"),
    "op_ccdecoder_1024": lambda c: F.test_ccdecoder_bit_exact(c.torch, c.capi, c.orc, 1024, 5, "noisy"),
    "op_ccdecoder_640": lambda c: F.test_ccdecoder_bit_exact(c.torch, c.capi, c.orc, 640, 7, "noisy"),
    "op_viterbi27": lambda c: F.test_viterbi27(c.torch, c.capi, c.orc, 40.0),
    "op_rs223_i4_dual": lambda c: F.test_rs_decode_matrix(c.torch, c.capi, c.orc, "rs223", 4, 1, -1),
    "op_rs239_i5_fill3": lambda c: F.test_rs_decode_matrix(c.torch, c.capi, c.orc, "rs239", 5, 1, 3),
}


@pytest.mark.parametrize("fill", [255, 127])
@pytest.mark.parametrize("family", list(FILLED))
def test_filled_blocks(ctx, family, fill):
    """Leg A: every block handed out is 0xFF.. or 0x7F.. -- as floats NaN and 3.4e38, as int8 -1 and +127, as counters and flags anything but the zero of a fresh page --
    and the family's own test still holds, against its oracle or golden file."""
    with _clean_state(ctx.capi):
        os.environ["SDHIP_ALLOC_FILL"] = str(fill)
        before = ctx.capi.pool_stats()
        FILLED[family](ctx)
        after = ctx.capi.pool_stats()
        handed = after.dev_fresh + after.pin_fresh - before.dev_fresh - before.pin_fresh
        assert after.filled - before.filled == handed > 0, (family, after.filled - before.filled, handed)


def test_fill_value_is_checked(ctx):
    """a value that is no byte is an error of the handle's creation, not a silent default"""
    with _clean_state(ctx.capi):
        os.environ["SDHIP_ALLOC_FILL"] = "0x1FF"
        with pytest.raises(ctx.capi.SdhipError, match="SDHIP_ALLOC_FILL"):
            _solo(lambda: _fec_open(ctx, "concat", "B"))


# ================================================================ Leg B: recycled blocks
RECYCLED = {
    # family: (opener(ctx, which), must own pinned buffers on this path). Whatever the flag says, a family whose first handle drew pinned blocks is held to recycling them.
    "psk_goes_chunked": (lambda c, w: _psk_open(c, "goes", w, exact=False), False),
    "psk_npp_exact": (lambda c, w: _psk_open(c, "npp", w, exact=True, cuts=[0, 100000, 250000, 400000]), False),
    "psk_goes_host": (lambda c, w: _psk_open(c, "goes", w, exact=False, host=True), True),
    "psk_npp_host": (lambda c, w: _psk_open(c, "npp", w, exact=False, host=True), True),  # (QPSK without the float symbols: k_compact8 writes the soft bytes)
    # (2.57 samples per symbol: the chunks' symbol counts, and with them where each row of k_compact8 ends, follow the timing loop and differ from stream to stream)
    "psk_metop_host": (lambda c, w: _psk_open(c, "metop", w, exact=False, host=True), True),
    "fec_concat": (lambda c, w: _fec_open(c, "concat", w), False),
    "fec_concat_host": (lambda c, w: _fec_open(c, "concat", w, host=True), True),
    "fec_metop": (lambda c, w: _fec_open(c, "metop", w), False),
    "fec_punctured": (lambda c, w: _fec_open(c, "punctured", w, host=True), True),
    "fec_simple_psk": (lambda c, w: _fec_open(c, "simple", w), False),
    "fsk_a": (lambda c, w: _fsk_open(c, "fsk_a", w), False),
    "sdpsk_c_host": (lambda c, w: _fsk_open(c, "sdpsk_c", w, host=True), True),
    "lrpt": (lambda c, w: _lrpt_open(c, w), False),
    "lrpt_host": (lambda c, w: _lrpt_open(c, w, host=True), False),  # (the LRPT decoder owns no pinned buffer: its push copies straight to the device)
    "fy3_ahrpt": (lambda c, w: _fec_open(c, "fy3", w), False),
    "fy3_mpt": (lambda c, w: _fec_open(c, "fy3_mpt", w), False),
    "ccsds_ldpc": (lambda c, w: _ccsds_open(c, "r78_qpsk_direct", w), False),
    "ccsds_ldpc_host": (lambda c, w: _ccsds_open(c, "r78_oqpsk_internal", w, host=True), True),
    "s2_ldpc_bch_short_1_2": (lambda c, w: _s2fec_open(c, 1, "1/2", w), False),
    "s2_ldpc_bch_normal_2_3": (lambda c, w: _s2fec_open(c, 0, "2/3", w), False),
    "s2_demod": (lambda c, w: _dvbs2_open(c, 12, 1, w), False),
    "ndsp_qpsk": (lambda c, w: _ndsp_open(c, w), False),
    "ndsp_costas_fast": (lambda c, w: _costas_fast_open(c, w), False),
}


def _delta(b, a):
    return {n: getattr(b, n) - getattr(a, n) for n in ("dev_fresh", "dev_recycled", "pin_fresh", "pin_recycled")}


@pytest.mark.parametrize("family", list(RECYCLED))
def test_recycled_blocks(ctx, family):
    """Leg B, the benchmark's configuration: handle 2 is built from the blocks handle 1 left, which hold another stream's intermediate and final results."""
    opener, pinned = RECYCLED[family]
    capi = ctx.capi
    with _clean_state(capi):
        want = _solo(lambda: opener(ctx, "B"))
        capi.pool_enable(True)
        s0 = capi.pool_stats()
        first = _solo(lambda: opener(ctx, "A"))
        assert _flat(first) != _flat(want), "stream A must not be stream B"
        s1 = capi.pool_stats()
        drew = _delta(s1, s0)
        assert drew["pin_fresh"] + drew["pin_recycled"] > 0 or not pinned, "the family was expected to own pinned buffers"
        pinned = drew["pin_fresh"] + drew["pin_recycled"] > 0
        assert s1.dev_parked > 0 and s1.dev_parked_bytes > 0, "handle 1 parked nothing"
        if pinned:
            assert s1.pin_parked > 0 and s1.pin_parked_bytes > 0, "handle 1 parked no pinned block"
        got = _solo(lambda: opener(ctx, "B"))
        d = _delta(capi.pool_stats(), s1)
        print(f"recycled_blocks[{family}]: handle 2 drew device blocks {d['dev_recycled']} recycled / {d['dev_fresh']} fresh, pinned {d['pin_recycled']} recycled / {d['pin_fresh']} fresh")
        assert d["dev_recycled"] > 0, "handle 2 recycled no device block: nothing was tested"
        if pinned:
            assert d["pin_recycled"] > 0, "handle 2 recycled no pinned block: nothing was tested"
        _assert_same(got, want, family)


GROWING = {
    # calls of n, 2 n and 4 n items; per path the kind of block a growing buffer must have released while the handle was alive. On the host path the demodulators gather
    # their input in the pinned staging buffers of HostPipe (4 MiB at first, doubled as the pushes need) and process it in one batch: there it is the pinned block that
    # grows; the LRPT and CCSDS LDPC decoders own no pinned buffer, their host entries grow the device buffers call by call like the device entries.
    "psk_goes": (lambda c, k: _psk_open(c, "goes", "B", exact=False, cuts=[0, 90000, 270000, 630000], host=k), {"dev": "dev", "host": "pin"}),
    "psk_npp_exact": (lambda c, k: _psk_open(c, "npp", "B", exact=True, cuts=[0, 90000, 270000, 630000], host=k), {"dev": "dev", "host": "pin"}),
    "fec_concat": (lambda c, k: _fec_open(c, "concat", "B", cuts=[0, 8192 * 2 + 5, 8192 * 6 + 15, 8192 * 14 + 35], host=k), {"dev": "dev", "host": "dev pin"}),
    "fsk_a": (lambda c, k: _fsk_open(c, "fsk_a", "B", cuts=[0, 9000, 27000, 63000], host=k), {"dev": "dev"}),
    "lrpt": (lambda c, k: _lrpt_open(c, "B", cuts=[0, 16384 + 5, 16384 * 3 + 15, 16384 * 7 + 35], host=k), {"dev": "dev", "host": "dev"}),
    "ccsds_ldpc": (lambda c, k: _ccsds_open(c, "r78_qpsk_direct", "B", cuts=[0, 8192 + 5, 8192 * 3 + 15, 8192 * 7 + 35], host=k), {"dev": "dev", "host": "dev"}),
}


@pytest.mark.parametrize("family,path", [(f, p) for f in GROWING for p in GROWING[f][1]])
def test_a_handle_that_grows(ctx, family, path):
    """Pool on, one handle, calls of n, 2 n and 4 n: every growth parks a block in the middle of the run, device or pinned, and a later reserve of the handle (or its
    worker thread's) may take a parked block straight back -- a pinned one at once, pin_free does not wait as dev_free does. The same calls with the pool off are
    the reference."""
    capi, host = ctx.capi, path == "host"
    opener, expect = GROWING[family][0], GROWING[family][1][path]
    with _clean_state(capi):
        want = _solo(lambda: opener(ctx, host))
        capi.pool_enable(True)
        s0 = capi.pool_stats()
        h = opener(ctx, host)
        seen = []
        h.before_destroy = lambda: seen.append(capi.pool_stats())
        for i in range(len(h.cuts) - 1):
            h.step(i)
        got = h.close()
        mid = seen[0]
        d = _delta(capi.pool_stats(), s0)
        print(f"a_handle_that_grows[{family}-{path}]: parked while alive {mid.dev_parked} device / {mid.pin_parked} pinned; drew {d}")
        if "dev" in expect:
            assert mid.dev_parked > 0, "no device block was released by a growing buffer while the handle was alive"
        if "pin" in expect:
            assert mid.pin_parked > 0, "no pinned block was released by a growing buffer while the handle was alive"
        _assert_same(got, want, family)


def test_pool_off_and_trim_leave_nothing_parked(ctx):
    capi = ctx.capi
    with _clean_state(capi):
        capi.pool_enable(True)
        _solo(lambda: _fec_open(ctx, "concat", "A", host=True))
        s = capi.pool_stats()
        assert s.dev_parked > 0 and s.pin_parked > 0 and s.dev_parked_bytes > 0 and s.pin_parked_bytes > 0
        capi.pool_trim()
        s = capi.pool_stats()
        assert (s.dev_parked, s.pin_parked, s.dev_parked_bytes, s.pin_parked_bytes) == (0, 0, 0, 0)
        _solo(lambda: _fec_open(ctx, "concat", "A", host=True))  # the pool is still on: this handle's blocks (all fresh: nothing was left) are parked again
        s2 = capi.pool_stats()
        assert s2.dev_recycled == s.dev_recycled and s2.pin_recycled == s.pin_recycled and s2.dev_parked > 0
        capi.pool_enable(False)
        s3 = capi.pool_stats()
        assert (s3.dev_parked, s3.pin_parked, s3.dev_parked_bytes, s3.pin_parked_bytes) == (0, 0, 0, 0)
        _solo(lambda: _fec_open(ctx, "concat", "B", host=True))
        s4 = capi.pool_stats()
        assert s4.dev_recycled == s3.dev_recycled and s4.pin_recycled == s3.pin_recycled and s4.dev_fresh > s3.dev_fresh and s4.pin_fresh > s3.pin_fresh
        assert (s4.dev_parked, s4.pin_parked) == (0, 0)


# ================================================================ Leg C: two live handles
def _alternate(open_a, open_b):
    a, b = open_a(), open_b()
    assert len(a.cuts) == len(b.cuts) == 4
    for i in range(3):
        a.step(i)
        b.step(i)
    return a.close(), b.close()


PAIRS = {
    "psk_goes_bpsk+psk_npp_qpsk": (lambda c: _psk_open(c, "goes", "B", exact=False), lambda c: _psk_open(c, "npp", "B", exact=False)),
    "fec_concat_rs223_dual+fec_tail_rs239": (lambda c: _fec_open(c, "concat", "B"), lambda c: _fec_open(c, "tail_rs239", "B")),
    "fec_metop+psk_goes": (lambda c: _fec_open(c, "metop", "B"), lambda c: _psk_open(c, "goes", "A", exact=False)),
    "s2_ldpc_bch_short_1_2+normal_2_3": (lambda c: _s2fec_open(c, 1, "1/2", "B"), lambda c: _s2fec_open(c, 0, "2/3", "B")),
    "ccsds_ldpc_qpsk_direct+oqpsk_internal": (lambda c: _ccsds_open(c, "r78_qpsk_direct", "B"), lambda c: _ccsds_open(c, "r78_oqpsk_internal", "B")),
    "s2_demod_8psk_3_5+qpsk_1_2": (lambda c: _dvbs2_open(c, 12, 1, "B"), lambda c: _dvbs2_open(c, 4, 1, "B")),
    "ndsp_qpsk+costas_fast": (lambda c: _ndsp_open(c, "B"), lambda c: _costas_fast_open(c, "A")),
    "fsk_a+sdpsk_c": (lambda c: _fsk_open(c, "fsk_a", "B"), lambda c: _fsk_open(c, "sdpsk_c", "B")),
    "lrpt+fy3_ahrpt": (lambda c: _lrpt_open(c, "B"), lambda c: _fec_open(c, "fy3", "B")),
}


@pytest.mark.parametrize("pair", list(PAIRS))
def test_two_live_handles(ctx, pair):
    """Leg C: both handles open, their calls alternated; what one leaves in anything they share (the pool's maps, the profiler's events, tables and scratch rows
    kept per device) must not reach the other: each equals its solo run over the same slices."""
    oa, ob = PAIRS[pair]
    with _clean_state(ctx.capi):
        want_a, want_b = _solo(lambda: oa(ctx)), _solo(lambda: ob(ctx))
        got_a, got_b = _alternate(lambda: oa(ctx), lambda: ob(ctx))
        _assert_same(got_a, want_a, pair + " (first handle)")
        _assert_same(got_b, want_b, pair + " (second handle)")


def test_bb_to_soft_alternating_modcods(ctx):
    """sdhip_s2_bb_to_soft_dev keeps one demapper table and scratch rows per device (S2DemapCache) and uploads the table again when its bytes change: two modcods with
    their two tables called alternately re-upload it on every call, and each call still gives what it gives alone."""
    if not pyref.S2FrontRef.available():
        pytest.skip("oracle/_ref/libsdref_dvbs2.so without the front-end entries")
    ref, lib = pyref.S2FrontRef(), ctx.capi.lib()
    cases = []
    for modcod, short, pilots in (G.BB2SOFT[3], G.BB2SOFT[1]):  # 8PSK 3/5 and QPSK 1/2, short frames
        c = ref.cfg(modcod, short, pilots)
        fr = dvbs2_util.plframes(c["slots"], (modcod << 2) | (short << 1) | pilots, 3, seed=modcod)
        cases.append((modcod, short, pilots, fr, ref.lut(modcod, short), c["slots"] * 90 * c["bits"]))

    def call(case, k):
        modcod, short, pilots, fr, lut, nsoft = case
        d_fr, d_soft, d_pls = ctx.to_dev(fr[k:k + 1].view(np.float32)), ctx.zeros_dev(nsoft, np.int8), ctx.zeros_dev(1, np.int32)
        rc = lib.sdhip_s2_bb_to_soft_dev(0, modcod, short, pilots, C.c_void_p(d_fr[1]), fr.shape[1], 1, lut.ctypes.data_as(C.c_void_p), 256, C.c_void_p(d_soft[1]), C.c_void_p(d_pls[1]))
        assert rc == nsoft, ctx.capi.last_error()
        return ctx.to_host(d_soft).copy(), ctx.to_host(d_pls).copy()

    with _clean_state(ctx.capi):
        want = [[call(case, k) for k in range(3)] for case in cases]
        assert not np.array_equal(cases[0][4], cases[1][4])
        got = [[None] * 3, [None] * 3]
        for k in range(3):
            for j in (0, 1):
                got[j][k] = call(cases[j], k)
        _assert_same(got, want, "bb_to_soft")
        for j in (0, 1):  # and against the reference block, frame by frame
            w, _ = ref.bb_to_soft(*cases[j][:3], cases[j][3])
            assert np.array_equal(np.stack([g[0] for g in got[j]]), w)


def test_two_live_handles_under_the_profiler(ctx):
    """the profiler's records and event pool are process-wide: with it on around an alternating pair the outputs stay what they are, and every kernel's launch count
    is the sum of the two solo runs"""
    capi = ctx.capi
    oa, ob = (lambda: _fec_open(ctx, "concat", "B")), (lambda: _psk_open(ctx, "goes", "B", exact=False))
    with _clean_state(capi):
        want_a, want_b = _solo(oa), _solo(ob)
        try:
            capi.prof_enable(True)
            counts = []
            for run in (lambda: _solo(oa), lambda: _solo(ob), lambda: _alternate(oa, ob)):
                capi.prof_reset()
                res = run()
                counts.append({k: v[1] for k, v in capi.prof_get().items()})
        finally:
            capi.prof_enable(False)
            capi.prof_reset()
        _assert_same(res[0], want_a, "fec under the profiler")
        _assert_same(res[1], want_b, "demod under the profiler")
        assert counts[0] and counts[1] and not set(counts[0]) <= set(counts[1])
        total = {k: counts[0].get(k, 0) + counts[1].get(k, 0) for k in set(counts[0]) | set(counts[1])}
        assert counts[2] == total
