"""GPU parity tests of ccsds_turbo_decoder (run with -m gpu; tests/test_ccsds_turbo_on_twin_cpu.py collects the same functions against the host twin). Every call
goes through the C ABI. The reference's behaviour reaches these tests as data: tests/golden/turbo/*.npz, recorded by tools/gen_ccsds_turbo_golden.py from the
reference's own CCSDSTurbo (over libturbocodes / libconvcodes), derand_ccsds_soft and GenericCRC behind a restatement of the module's loop.

Held bit for bit: descriptors (offset, pos, swapped, correlation, CRC), output bytes, statistics, the interleavers, the per-position correlation, and the unit
decode's bits wherever the reference decodes a CRC-good frame. The a-priori arrays of one BCJR pass are doubles that went through exp / log: on the host twin, which
links the libm the fixtures were recorded with, they are held bit for bit; on the GPU to BCJR_TOLERANCE (the device's exp / log are not glibc's)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "turbo")
STREAMS = ["r12_b223", "r13_b223", "r14_b223", "r16_b223"]
# five frames of a longer block each, inside the waterfall, turbo_iters = 5: what they emit depends on the iteration count (test_stream_needs_its_iterations)
LONG_STREAMS = ["r13_b446", "r14_b892", "r12_b1115"]
BACKEND = "gpu"  # the twin's collection sets "twin"
# max |ours - fixture| / max(1, |fixture|) over the two BCJR fixtures as first measured on an MI355X (profiles/ccsds_turbo_bench.json); the test
# allows 16 times that, and never more than 1e-9
BCJR_MEASURED = 1.665e-15
BCJR_TOLERANCE = min(16 * BCJR_MEASURED, 1e-9)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def capi():
    import torch
    if torch.cuda.is_available():  # torch's HIP runtime first, as in tests/test_lrpt_gpu.py: the library then binds to the one already loaded
        torch.zeros(1, device="cuda")
    from satdump_amd import capi as c
    c.lib()
    return c


_cache = {}


def _golden(name):
    if name not in _cache:
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        g = {k: z[k] for k in z.files}
        if "params" in g:
            g["params"] = json.loads(bytes(g["params"]).decode())
        for a in g.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = g
    return _cache[name]


def _dev(torch, a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()  # (a copy: the fixtures' arrays are read-only)


def _cfg(capi, g, **over):
    p = g["params"]
    kw = dict(rate=p["turbo_rate"], base=p["turbo_base"], iterations=p["turbo_iters"])
    kw.update(over)
    return capi.ccsds_turbo_cfg(**kw)


def _run(torch, capi, g, bounds, **over):
    """the fixture's stream through a fresh handle in the calls `bounds` cuts it into: (output bytes, descriptors, statistics)"""
    dec = capi.CcsdsTurbo(_cfg(capi, g, **over))
    F = g["params"]["F"]
    d_x = _dev(torch, g["soft"])
    out, descs = [], []
    for a, b in zip(bounds[:-1], bounds[1:]):
        cap = (b - a) // F + 4
        d_out = _dev(torch, np.zeros(cap * dec.frame_bytes, np.uint8))
        k = dec.process_dev(d_x.data_ptr() + a, b - a, d_out.data_ptr(), cap)
        out.append(d_out.cpu().numpy()[: k * dec.frame_bytes])
        descs.append(dec.descs())
    st = dec.stats()
    dec.close()
    return np.concatenate(out), np.concatenate(descs), st


def _check(g, out, descs, st):
    for name in ("offset", "pos", "swapped", "crc_ok"):
        assert np.array_equal(descs[name].astype(np.int64), np.asarray(g[name]).astype(np.int64)), name
    assert np.array_equal(descs["cor"].view(np.uint32), np.asarray(g["cor"]).view(np.uint32))
    want = np.asarray(g["out"])
    assert len(out) == len(want) and np.array_equal(out, want)
    assert st.reads == len(g["offset"]) and st.soft_in == len(g["soft"]) and st.frames_out * (g["params"]["turbo_base"] + 4) == len(want)
    assert st.locked == int(g["stats"][0]) and st.crc_lock == int(g["stats"][1])
    assert np.float32(st.cor).view(np.uint32) == np.asarray(g["stat_cor"]).view(np.uint32)[0]


def test_defaults(capi):
    """needs no device: the defaults, the ASM tables, the interleavers of the four bases"""
    c = capi.ccsds_turbo_cfg()
    assert (c.rate, c.base, c.iterations, c.device) == (capi.CCSDS_TURBO_RATES["1/2"], 223, 10, 0)
    for name in STREAMS:
        g = _golden(name)
        a = np.zeros(192, np.float32)
        n = capi.lib().sdhip_ccsds_turbo_asm(capi.CCSDS_TURBO_RATES[g["params"]["turbo_rate"]], a.ctypes.data_as(C.c_void_p))
        assert n == len(g["asm"]) and np.array_equal(a[:n].view(np.uint32), np.asarray(g["asm"]).view(np.uint32)), name
    u = _golden("turbo_unit")
    for base in (223, 446, 892, 1115):
        pi = capi.ccsds_turbo_interleaver(base)
        assert np.array_equal(pi, np.asarray(u[f"pi_{base}"]).astype(np.int32)), base
    assert capi.lib().sdhip_ccsds_turbo_interleaver(224, None) < 0 and "223, 446, 892 or 1115" in capi.last_error()


@gpu
def test_refusals(capi):
    g = _golden("r12_b223")
    for over, msg in ((dict(rate="1/5"), "Invalid Turbo Rate"), (dict(rate=4), "Invalid Turbo Rate"), (dict(base=224), "223, 446, 892 or 1115"), (dict(base=0), "223, 446, 892 or 1115"),
                      (dict(iterations=0), "turbo_iters"), (dict(iterations=-3), "turbo_iters")):
        h = capi.lib().sdhip_ccsds_turbo_create(C.byref(_cfg(capi, g, **over)))
        assert not h, over
        assert msg in capi.last_error(), (over, capi.last_error())
    assert capi.lib().sdhip_op_ccsds_turbo_decode(0, 7, 223, 2, None, 0, None) < 0 and "Invalid Turbo Rate" in capi.last_error()
    assert capi.lib().sdhip_op_ccsds_turbo_decode(0, 0, 500, 2, None, 0, None) < 0 and "223, 446, 892 or 1115" in capi.last_error()
    assert capi.lib().sdhip_op_ccsds_turbo_decode(0, 0, 223, 0, None, 0, None) < 0 and "turbo_iters" in capi.last_error()
    assert capi.lib().sdhip_op_ccsds_turbo_bcjr(0, 0, 223, 2, None, 0, None) < 0 and "constituent" in capi.last_error()


@gpu
@pytest.mark.parametrize("name", ["r12_b223", "r16_b223"])
def test_unit_correlator_bit_exact(torch_cuda, capi, name):
    """per position of the first two reads' bytes (64 and 192 taps): the float bits of the module's dot product"""
    g = _golden(name)
    rate = capi.CCSDS_TURBO_RATES[g["params"]["turbo_rate"]]
    head = np.asarray(g["soft"])[: 2 * g["params"]["F"]]
    n, m = len(head), len(g["pos_cor"])
    d_x = _dev(torch_cuda, head)
    d_cor = _dev(torch_cuda, np.zeros(n, np.float32))
    k = capi.lib().sdhip_op_ccsds_turbo_correlate(0, rate, d_x.data_ptr(), n, d_cor.data_ptr())
    assert k == m == n - len(g["asm"]) + 1, capi.last_error()
    assert np.array_equal(d_cor.cpu().numpy()[:m].view(np.uint32), np.asarray(g["pos_cor"]).view(np.uint32))


def _message_error(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


@gpu
@pytest.mark.parametrize("tag", ["bcjr_r12", "bcjr_r16"])
def test_bcjr_unit(torch_cuda, capi, tag):
    """one convcode_extrinsic pass of the upper code from log(0.5), one of the lower code on the interleaved result: the a-priori arrays it leaves"""
    u = _golden("turbo_unit")
    rate = capi.CCSDS_TURBO_RATES["1/2" if tag.endswith("12") else "1/6"]
    L = 223 * 8
    worst = 0.0
    for code, stream, start, want in ((0, u[tag + "_stream0"], np.full((2, L), np.log(0.5)), u[tag + "_after_upper"]), (1, u[tag + "_stream1"], u[tag + "_lower_in"], u[tag + "_after_lower"])):
        d_s = _dev(torch_cuda, np.asarray(stream, np.float64))
        d_m = _dev(torch_cuda, np.asarray(start, np.float64))
        rc = capi.lib().sdhip_op_ccsds_turbo_bcjr(0, rate, 223, code, d_s.data_ptr(), 1, d_m.data_ptr())
        assert rc == 0, capi.last_error()
        got, want = d_m.cpu().numpy(), np.asarray(want)
        assert got.shape == want.shape and np.isfinite(got).all()
        err = _message_error(got, want)
        worst = max(worst, err)
        print(f"{tag} code {code}: max |ours - fixture| / max(1, |fixture|) = {err:.3e}, {int((got.view(np.uint64) != want.view(np.uint64)).sum())} of {got.size} doubles differ")
        if BACKEND == "twin":
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (tag, code, err)
        else:
            assert err <= BCJR_TOLERANCE, (tag, code, err)
    print(f"{tag}: worst {worst:.3e}")


UNIT = [("dec_b446_r13", "1/3", 446), ("dec_b892_r14", "1/4", 892), ("dec_b1115_r16", "1/6", 1115)]


def _unit_decode(torch, capi, rate, base, iterations, soft):
    cw = np.asarray(soft).astype(np.float32) * np.float32(1.0 / 127.0)  # what the module hands CCSDSTurbo::decode
    n = len(cw)
    d_cw = _dev(torch, cw)
    d_bits = _dev(torch, np.full(n * base * 8, 7, np.uint8))
    rc = capi.lib().sdhip_op_ccsds_turbo_decode(0, capi.CCSDS_TURBO_RATES[rate], base, iterations, d_cw.data_ptr(), n, d_bits.data_ptr())
    assert rc == 0, capi.last_error()
    bits = d_bits.cpu().numpy().reshape(n, base * 8)
    assert bits.max() <= 1
    return bits


@gpu
@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("tag,rate,base", UNIT)
def test_unit_decode(torch_cuda, capi, tag, rate, base, iterations):
    """CCSDSTurbo::decode's bits in front of the CRC gate: identical wherever the reference decodes a CRC-good frame (the transmitted one); for a codeword it does
    not decode, the number of differing bits is printed -- and on the host twin, whose arithmetic is the reference's, that number is held to 0 as well. (On the
    GPU the bits of codewords inside the waterfall are held by tests/test_ccsds_turbo_waterfall_gpu.py, wherever the reference's own bits are stable.)"""
    u = _golden("turbo_unit")
    want = np.unpackbits(np.asarray(u[f"{tag}_bits_{iterations}"]), axis=1)
    sent = np.asarray(u[tag + "_sent"])
    bits = _unit_decode(torch_cuda, capi, rate, base, iterations, u[tag + "_cw"])
    good = (want == sent).all(1)
    assert good.any() or iterations == 1, tag
    for k in range(len(want)):
        diff = int((bits[k] != want[k]).sum())
        print(f"{tag}[{k}] after {iterations} iterations: the reference decodes the transmitted frame: {bool(good[k])}; {diff} of {base * 8} bits differ from the reference's")
        if good[k] or BACKEND == "twin":
            assert diff == 0, (tag, k, diff)


@gpu
def test_unit_decode_rails(torch_cuda, capi):
    """a codeword of soft bytes over the whole int8 range, -128 and 127 among them"""
    u = _golden("turbo_unit")
    soft = np.asarray(u["rails_cw"])
    assert (soft == -128).sum() >= 20 and (soft == 127).sum() >= 20
    bits = _unit_decode(torch_cuda, capi, "1/3", 223, 2, soft)
    assert np.array_equal(np.packbits(bits, axis=1), u["rails_bits_2"])


@gpu
@pytest.mark.parametrize("name", STREAMS + LONG_STREAMS)
def test_stream_one_call(torch_cuda, capi, name):
    g = _golden(name)
    _check(g, *_run(torch_cuda, capi, g, [0, len(g["soft"])]))


@gpu
@pytest.mark.parametrize("name", STREAMS + LONG_STREAMS)
def test_stream_three_calls(torch_cuda, capi, name):
    g = _golden(name)
    n = len(g["soft"])
    _check(g, *_run(torch_cuda, capi, g, [0, n // 3 + 17, 2 * n // 3 + 401, n]))


def _ragged(g):
    """empty, 1-byte and F - 1-byte calls in between (in stream order: the five-frame streams end before 4 F + 100 + n // 2)"""
    n, F = len(g["soft"]), g["params"]["F"]
    return sorted([0, 0, 1, F, F, 2 * F - 1, 2 * F, 4 * F + 100, 4 * F + 101, n // 2, n // 2 + F - 1, n - 1, n, n])


@gpu
@pytest.mark.parametrize("name", STREAMS + LONG_STREAMS)
def test_stream_ragged_calls(torch_cuda, capi, name):
    """empty, 1-byte and F - 1-byte calls in between: an incomplete read, and an incomplete slide, stay pending"""
    g = _golden(name)
    _check(g, *_run(torch_cuda, capi, g, _ragged(g)))


@gpu
@pytest.mark.parametrize("name", ["r13_b223", "r14_b223"])
def test_host_push_pull_path(capi, name):
    """push / pull with host buffers == the device path"""
    g = _golden(name)
    dec = capi.CcsdsTurbo(_cfg(capi, g))
    soft = np.asarray(g["soft"])
    got = []
    for a in range(0, len(soft), 20001):
        dec.push(soft[a:a + 20001])
        got.append(dec.pull(2))
    got.append(dec.pull())
    st = dec.stats()
    dec.close()
    assert np.array_equal(np.concatenate(got).reshape(-1), np.asarray(g["out"]))
    assert st.reads == len(g["offset"])


@gpu
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", STREAMS)
def test_statistics_inside_a_slide(torch_cuda, capi, name, which):
    """a stream that ends inside a slide's extra read (the first read's, and the sidelobe slide's behind the dropped bytes): the module has set locked / cor when
    it asks for the bytes; the buffer is not decoded yet"""
    g = _golden(name)
    tl = int(g["trunc_len"][which])
    dec = capi.CcsdsTurbo(_cfg(capi, g))
    d_x = _dev(torch_cuda, np.asarray(g["soft"])[:tl])
    cap = tl // g["params"]["F"] + 4
    d_out = _dev(torch_cuda, np.zeros(cap * dec.frame_bytes, np.uint8))
    dec.process_dev(d_x.data_ptr(), tl, d_out.data_ptr(), cap)
    st = dec.stats()
    nd = len(dec.descs())
    dec.close()
    assert st.locked == int(g["trunc_stats"][which][0]) == 0
    assert np.float32(st.cor).view(np.uint32) == np.asarray(g["trunc_cor"]).view(np.uint32)[which]
    assert st.reads == nd == int(g["trunc_reads"][which])
    if nd:
        assert st.crc_lock == int(g["trunc_stats"][which][1])
