"""GPU parity tests of ccsds_ldpc_decoder, "ldpc_rate": "7/8" (run with -m gpu; tests/test_ccsds_ldpc_on_twin_cpu.py collects the same functions against the host
twin). Every call goes through the C ABI. The reference's behaviour reaches these tests as data: tests/golden/ldpc/*.npz, recorded by
tools/gen_ccsds_ldpc_golden.py from the reference's own CorrelatorGeneric, rotate_soft, derand_ccsds_soft, CCSDSLDPC over LDPCDecoderGeneric and
BPSK_CCSDS_Deframer. Everything is held bit for bit: descriptors (offset, syncword, correlation, corrections, lock), output bytes, statistics."""
import ctypes as C
import json
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu  # every test but test_defaults needs the device
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ldpc")
STREAMS = ["r78_qpsk_direct", "r78_oqpsk_internal", "r78_bpsk", "r78_noise", "r78_rails"]
# four frames each: shorter than the byte positions the ragged cut is written for, so they take the one-call, three-call and correlator tests only
SHORT_RAILS = ["r78_rails_oqpsk", "r78_rails_bpsk"]
F, CW, DATA = 8192, 8160, 7136


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def capi():
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
    kw = dict(constellation=p["constellation"], rate="7/8", iterations=p["iterations"], derandomize=p["derandomize"], internal_stream=p["internal_stream"],
              internal_cadu_size=p.get("internal_cadu_size", 0), internal_asm=p.get("internal_asm", 0x1ACFFC1D))
    kw.update(over)
    return capi.ccsds_ldpc_cfg(**kw)


def _expected(g):
    """(output bytes, deframer state or None) of the fixture"""
    return np.asarray(g["out"]), (int(g["stats"][2]) if g["params"]["internal_stream"] else None)


def _run(torch, capi, g, bounds):
    """the fixture's stream through a fresh handle in the calls `bounds` cuts it into: (output bytes, descriptors, statistics)"""
    dec = capi.CcsdsLdpc(_cfg(capi, g))
    soft = g["soft"]
    d_x = _dev(torch, soft)
    out, descs = [], []
    for a, b in zip(bounds[:-1], bounds[1:]):
        cap = (b - a) // F + 4
        d_out = torch.zeros(cap * dec.frame_bytes, dtype=torch.uint8, device="cuda")
        k = dec.process_dev(d_x.data_ptr() + a, b - a, d_out.data_ptr(), cap)
        out.append(d_out[: k * dec.frame_bytes].cpu().numpy())
        descs.append(dec.descs())
    st = dec.stats()
    dec.close()
    return np.concatenate(out), np.concatenate(descs), st


def _check(g, out, descs, st):
    for k, name in (("offset", "offset"), ("sync", "sync"), ("corrections", "corrections"), ("locked", "locked")):
        assert np.array_equal(descs[name].astype(np.int64), np.asarray(g[k]).astype(np.int64)), name
    assert np.array_equal(descs["cor"].view(np.uint32), np.asarray(g["cor"]).view(np.uint32))
    want, state = _expected(g)
    assert len(out) == len(want) and np.array_equal(out, want)
    assert st.frames_seen == len(g["offset"]) and st.soft_in == len(g["soft"])
    assert st.correlator_lock == int(g["stats"][0]) and st.ldpc_corr == int(g["stats"][1])
    assert np.float32(st.correlator_corr).view(np.uint32) == np.asarray(g["stat_cor"]).view(np.uint32)[0]
    if state is not None:
        assert st.deframer_state == state


def test_defaults(capi):
    """needs no device: the defaults of the module's optional keys, the frame sizes' constants, the correlator's tables"""
    c = capi.ccsds_ldpc_cfg()
    assert (c.derandomize, c.internal_stream, c.block_size, c.internal_asm, c.rate) == (1, 0, 0, 0x1ACFFC1D, capi.CCSDS_LDPC_RATES["7/8"])
    for name in ("r78_qpsk_direct", "r78_oqpsk_internal", "r78_bpsk"):
        g = _golden(name)
        sw = np.zeros((4, 32), np.float32)
        n = capi.lib().sdhip_ccsds_ldpc_syncwords(g["params"]["constellation"], sw.ctypes.data_as(C.c_void_p))
        assert n == len(g["syncwords"]) and np.array_equal(sw[:n].view(np.uint32), np.asarray(g["syncwords"]).view(np.uint32)), name


@gpu
@pytest.mark.parametrize("iterations", [1, 10, 25])
def test_unit_decode_bit_exact(torch_cuda, capi, iterations):
    g = _golden("r78_unit")
    cw = g["codewords"]
    n = len(cw)
    d_cw = _dev(torch_cuda, cw)
    d_bits = torch_cuda.zeros(n * CW, dtype=torch_cuda.uint8, device="cuda")
    d_corr = torch_cuda.zeros(n, dtype=torch_cuda.int32, device="cuda")
    rc = capi.lib().sdhip_op_ccsds_ldpc_decode(0, capi.CCSDS_LDPC_RATES["7/8"], iterations, d_cw.data_ptr(), n, d_bits.data_ptr(), d_corr.data_ptr())
    assert rc == 0, capi.last_error()
    bits = d_bits.cpu().numpy().reshape(n, CW)
    assert bits.max() <= 1
    assert np.array_equal(np.packbits(bits, axis=1), g[f"bits_{iterations}"])
    assert np.array_equal(d_corr.cpu().numpy(), g[f"corrections_{iterations}"])


@gpu
@pytest.mark.parametrize("iterations", [1, 10])
def test_unit_decode_rails(torch_cuda, capi, iterations):
    """prepared codewords quantised to the whole int8 range, 7 % of them -128 (what the soft derandomiser makes of a 127): bits and return values of CCSDSLDPC::decode"""
    g = _golden("r78_rails")
    cw = g["rails_codewords"]
    n = len(cw)
    assert (np.asarray(cw) == -128).mean() >= 0.05
    right = {it: (np.asarray(g[f"rails_bits_{it}"]) == np.asarray(g["rails_words"])).all(1) for it in (1, 10)}  # by the fixture alone: the words are decodable, not trivially
    assert right[10].sum() >= 4 and (right[10] & ~right[1]).any()
    d_cw = _dev(torch_cuda, cw)
    d_bits = torch_cuda.zeros(n * CW, dtype=torch_cuda.uint8, device="cuda")
    d_corr = torch_cuda.zeros(n, dtype=torch_cuda.int32, device="cuda")
    rc = capi.lib().sdhip_op_ccsds_ldpc_decode(0, capi.CCSDS_LDPC_RATES["7/8"], iterations, d_cw.data_ptr(), n, d_bits.data_ptr(), d_corr.data_ptr())
    assert rc == 0, capi.last_error()
    bits = d_bits.cpu().numpy().reshape(n, CW)
    assert bits.max() <= 1
    assert np.array_equal(np.packbits(bits, axis=1), g[f"rails_bits_{iterations}"])
    assert np.array_equal(d_corr.cpu().numpy(), g[f"rails_corrections_{iterations}"])


@gpu
@pytest.mark.parametrize("name", STREAMS + SHORT_RAILS)
def test_unit_correlator_bit_exact(torch_cuda, capi, name):
    """per position of the first four frames: the correlation (float bits) and the syncword index -- which also proves the tables' six phasor literals"""
    g = _golden(name)
    head = np.asarray(g["soft"])[: 4 * F]
    n = len(head)
    d_x = _dev(torch_cuda, head)
    d_cor = torch_cuda.zeros(n, dtype=torch_cuda.float32, device="cuda")
    d_idx = torch_cuda.zeros(n, dtype=torch_cuda.uint8, device="cuda")
    k = capi.lib().sdhip_op_generic_correlate(0, g["params"]["constellation"], d_x.data_ptr(), n, d_cor.data_ptr(), d_idx.data_ptr())
    assert k == n - 31, capi.last_error()
    m = len(g["pos_cor"])
    assert m == n - 32
    assert np.array_equal(d_cor.cpu().numpy()[:m].view(np.uint32), np.asarray(g["pos_cor"]).view(np.uint32))
    assert np.array_equal(d_idx.cpu().numpy()[:m], g["pos_sync"])


@gpu
@pytest.mark.parametrize("name", STREAMS + SHORT_RAILS)
def test_stream_one_call(torch_cuda, capi, name):
    g = _golden(name)
    _check(g, *_run(torch_cuda, capi, g, [0, len(g["soft"])]))


@gpu
@pytest.mark.parametrize("name", STREAMS + SHORT_RAILS)
def test_stream_three_calls(torch_cuda, capi, name):
    g = _golden(name)
    n = len(g["soft"])
    _check(g, *_run(torch_cuda, capi, g, [0, n // 3 + 17, 2 * n // 3 + 4001, n]))


@gpu
@pytest.mark.parametrize("name", STREAMS)
def test_stream_ragged_calls(torch_cuda, capi, name):
    """empty, 1-byte and 8191-byte calls in between: an incomplete read, and an incomplete slide, stay pending"""
    g = _golden(name)
    n = len(g["soft"])
    b = [0, 0, 1, 8192, 8192, 16383, 16384, 40000, 40001, n // 2, n // 2 + 8191, n - 1, n, n]
    _check(g, *_run(torch_cuda, capi, g, b))


@gpu
@pytest.mark.parametrize("name", ["r78_qpsk_direct", "r78_oqpsk_internal"])
def test_host_push_pull_path(capi, name):
    """push / pull with host buffers == the device path"""
    g = _golden(name)
    dec = capi.CcsdsLdpc(_cfg(capi, g))
    soft = np.asarray(g["soft"])
    got = []
    for a in range(0, len(soft), 50001):
        dec.push(soft[a:a + 50001])
        got.append(dec.pull(5))
    got.append(dec.pull())
    dec.close()
    want, _ = _expected(g)
    assert np.array_equal(np.concatenate(got).reshape(-1), want)


@gpu
def test_noise_stream_terminates(torch_cuda, capi):
    """random soft bytes: the chain slides at every read, runs out of speculation rounds and finishes on the serial walk -- the fixture's frames, no more"""
    g = _golden("r78_noise")
    assert (np.asarray(g["locked"]) == 0).all()
    out, descs, st = _run(torch_cuda, capi, g, [0, len(g["soft"])])
    _check(g, out, descs, st)
    assert st.chain_serial >= 1 and st.frames_out == len(g["offset"])


@gpu
@pytest.mark.parametrize("name", ["r78_qpsk_direct", "r78_oqpsk_internal", "r78_noise"])
def test_statistics_inside_a_slide(torch_cuda, capi, name):
    """a stream that ends inside a slide's extra read: the module has set correlator_lock / correlator_corr at correlate() already, the frame is not decoded yet"""
    g = _golden(name)
    tl = int(g["trunc_len"][0])
    dec = capi.CcsdsLdpc(_cfg(capi, g))
    d_x = _dev(torch_cuda, np.asarray(g["soft"])[:tl])
    cap = tl // F + 4
    d_out = torch_cuda.zeros(cap * dec.frame_bytes, dtype=torch_cuda.uint8, device="cuda")
    dec.process_dev(d_x.data_ptr(), tl, d_out.data_ptr(), cap)
    st = dec.stats()
    dec.close()
    assert st.correlator_lock == int(g["trunc_stats"][0]) == 0
    assert np.float32(st.correlator_corr).view(np.uint32) == np.asarray(g["trunc_cor"]).view(np.uint32)[0]
    if st.frames_seen:
        assert st.ldpc_corr == int(g["trunc_stats"][1])
    assert st.frames_seen == int((np.asarray(g["offset"]) + F <= tl).sum())


@gpu
def test_level_schedule(capi):
    """the schedule computed from the row list is one a sequential pass over the rows allows: every row once; rows of a level share no variable node (they run
    between the same two barriers); and every variable node meets its rows in ascending row order, which is all the reference's order binds"""
    g = _golden("r78_bpsk")
    rows = np.asarray(_golden("r78_unit")["rows"]).astype(np.int64)
    dec = capi.CcsdsLdpc(_cfg(capi, g))
    lv, order = dec.levels(), dec.schedule().astype(np.int64)
    dec.close()
    assert sum(lv) == 1022 and all(x > 0 for x in lv) and sorted(order.tolist()) == list(range(1022))
    last_row = np.full(8176, -1, np.int64)
    a = 0
    for n in lv:
        level_rows = order[a:a + n]
        cols = rows[level_rows].reshape(-1)
        assert len(np.unique(cols)) == len(cols)  # no variable node twice inside a level
        for r in level_rows:
            assert (last_row[rows[r]] < r).all()
            last_row[rows[r]] = r
        a += n


@gpu
@pytest.mark.parametrize("iterations", [1, 6])
def test_generic_row_list_decode(torch_cuda, capi, iterations):
    """the engine on another row list -- 40 check nodes of 3 .. 9 edges, odd degrees among them (the parity's complement, ldpc_decoder_generic.cpp:133-134), rows
    shorter than the 32 lanes -- against LDPCDecoderGeneric on that list"""
    g = _golden("r78_unit")
    rows, nvn, words = np.ascontiguousarray(g["g_rows"]), int(g["g_nvn"][0]), g["g_words"]
    n = len(words)
    d_w = _dev(torch_cuda, words)
    d_bits = torch_cuda.zeros(n * nvn, dtype=torch_cuda.uint8, device="cuda")
    d_corr = torch_cuda.zeros(n, dtype=torch_cuda.int32, device="cuda")
    rc = capi.lib().sdhip_op_ldpc_generic_decode(0, rows.ctypes.data_as(C.c_void_p), len(rows), nvn, iterations, d_w.data_ptr(), n, d_bits.data_ptr(), d_corr.data_ptr())
    assert rc == 0, capi.last_error()
    assert np.array_equal(d_bits.cpu().numpy().reshape(n, nvn), g[f"g_bits_{iterations}"])
    assert np.array_equal(d_corr.cpu().numpy(), g[f"g_corrections_{iterations}"])


@gpu
def test_refusals(capi):
    g = _golden("r78_oqpsk_internal")
    for over, msg in ((dict(rate="1/2"), "7/8"), (dict(rate="2/3"), "7/8"), (dict(rate="4/5"), "7/8"), (dict(internal_cadu_size=8275), "padded"),
                      (dict(constellation="8psk"), "invalid constellation"), (dict(iterations=-1), "ldpc_iterations")):
        h = capi.lib().sdhip_ccsds_ldpc_create(C.byref(_cfg(capi, g, **over)))
        assert not h, over
        assert msg in capi.last_error(), (over, capi.last_error())
    rc = capi.lib().sdhip_op_ccsds_ldpc_decode(0, capi.CCSDS_LDPC_RATES["1/2"], 10, None, 0, None, None)
    assert rc < 0 and "7/8" in capi.last_error()
