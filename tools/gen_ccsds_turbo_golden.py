#!/usr/bin/env python3
"""tools/gen_ccsds_turbo_golden.py -- records what the reference's ccsds_turbo_decoder computes as fixtures under tests/golden/turbo/.

Needs the reference tree (REF, default /root/reference), gcc and g++; the tests that read the fixtures need none of them. The driver
tools/ccsds_turbo_golden_driver.cpp is compiled with the reference's own sources (CCSDSTurbo over libturbocodes.c / libconvcodes.c, derand_ccsds_soft, GenericCRC),
compiled where they lie, into a TEMPORARY directory with the oracle's recorded flags (-O2 -ffp-contract=off, ref_shim/); nothing compiled stays behind.

The streams are built here: frames of `base` bytes with a valid CRC-16, their codewords from CCSDSTurbo::encode, the wire format around them (ASM, randomiser, BPSK
soft bytes, AWGN) and the damage each case is about. tests/golden/turbo/INDEX.txt lists the files. Every stream file (base 223, one per rate) holds
    soft                      the input (int8)
    params                    JSON: the module's keys and how the stream was made
    offset, pos, swapped, cor, crc_ok      one entry per buffer the module decoded (stream position where its read started, where that read found the ASM, ...)
    out                       the bytes the module writes (frames of base + 4 bytes, CRC-good buffers only)
    stats, stat_cor           int32 {locked, crc_lock, 0} and float32 cor behind the whole stream
    trunc_len, trunc_stats, trunc_cor, trunc_reads   the same behind the stream's first trunc_len bytes, which end inside a slide's extra read
    asm                       the module's ASM table (float32)
    pos_cor                   the module's correlation at every position of the first two reads' bytes
turbo_unit.npz holds d_pi for the four bases; for base 223 at rates 1/2 and 1/6 one prepared codeword each with the two constituent streams and the a-priori
arrays after the first upper pass, in front of and after the first lower pass (convcode_extrinsic called directly); two prepared codewords each of (446, 1/3),
(892, 1/4) and (1115, 1/6) with CCSDSTurbo::decode's bits after 1 and 2 iterations and the transmitted bits; and `rails_*`: rate 1/3 base 223 codewords made of
soft bytes over the whole int8 range, -128 and 127 among them, with the bits after 2 iterations.

The generator asserts, and fails otherwise: every stream has a slide with pos > F / 2 (the start mid-frame), five bytes dropped early in a frame (the
read stays in lock on a shifted codeword; the next one cannot see the following ASM and slides to a sidelobe with pos <= F / 2: the stale-middle buffer, whose
CRC fails), swapped buffers, six buffers with at least 20 hard-decision errors each that decode to the transmitted frame, a codeword buried in noise and a
clean frame with one bit flipped whose CRC fails; the set of frames emitted is the same at turbo_iters and at turbo_iters - 1
and at least half of the frames sent are emitted; the output is the same for three cuttings of each stream."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CPP = ["common/codings/turbo/ccsds_turbo.cpp", "common/codings/randomization.cpp", "common/codings/crc/crc_generic.cpp"]
REF_C = ["libs/deepspace-turbo/libturbocodes.c", "libs/deepspace-turbo/libconvcodes.c"]
RATES = {"1/2": 0, "1/3": 1, "1/4": 2, "1/6": 3}
ASM_HEX = ["034776C7272895B0", "25D5C0CE8990F6C9461BF79C", "034776C7272895B0FCB88938D8D76A4F", "25D5C0CE8990F6C9461BF79CDA2A3F31766F0936B9E40863"]
WIRE = [2, 3, 4, 6]


def build_driver(ref: str, tmp: str) -> C.CDLL:
    sc = os.path.join(ref, "src-core")
    common = ["-O2", "-fPIC", "-ffp-contract=off", "-w", "-I" + sc]
    objs = []
    for f in REF_C:
        o = os.path.join(tmp, os.path.basename(f) + ".o")
        subprocess.check_call(["gcc"] + common + ["-c", os.path.join(sc, f), "-o", o])
        objs.append(o)
    flags = ["-std=c++17", "-DSOURCE_PATH_SIZE=0", "-I" + os.path.join(ROOT, "ref_shim"), "-fno-access-control", "-Dvolk_8i_s32f_convert_32f=volk_8i_s32f_convert_32f_u"]
    lib = os.path.join(tmp, "libturboref.so")
    subprocess.check_call(["g++"] + common + flags + ["-shared", "-o", lib, os.path.join(ROOT, "tools", "ccsds_turbo_golden_driver.cpp")] + [os.path.join(sc, f) for f in REF_CPP] +
                          objs + ["-lpthread", "-lm"])
    L = C.CDLL(lib)
    L.turboref_create.restype = C.c_void_p
    L.turboref_create.argtypes = [C.c_int, C.c_int, C.c_int]
    L.turboref_destroy.argtypes = [C.c_void_p]
    L.turboref_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    for f in ("turboref_ndesc", "turboref_nout"):
        getattr(L, f).restype = C.c_int64
        getattr(L, f).argtypes = [C.c_void_p]
    L.turboref_frame_size.argtypes = [C.c_void_p]
    L.turboref_results.argtypes = [C.c_void_p] * 9
    L.turboref_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.turboref_asm.argtypes = [C.c_void_p, C.c_void_p]
    L.turboref_pi.argtypes = [C.c_int, C.c_void_p]
    L.turboref_codeword_length.argtypes = [C.c_int, C.c_int]
    L.turboref_encode.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.turboref_decode.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.turboref_bcjr.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 6
    return L


def crc16(data: bytes) -> int:
    crc = 0xFFFF
    for b in data:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def make_frame(rng, base: int) -> np.ndarray:
    body = rng.integers(0, 256, base - 2).astype(np.uint8)
    c = crc16(body.tobytes())
    return np.concatenate([body, np.array([c >> 8, c & 0xFF], np.uint8)])


def soft_pn() -> np.ndarray:
    reg, out = 0xFF, []
    for _ in range(255):
        out.append(reg & 1)
        fb = (reg ^ (reg >> 3) ^ (reg >> 5) ^ (reg >> 7)) & 1
        reg = (reg >> 1) | (fb << 7)
    return np.array(out, dtype=np.uint8)


def asm_bits(rate: int) -> np.ndarray:
    return np.array([(int(ch, 16) >> (3 - k)) & 1 for ch in ASM_HEX[rate] for k in range(4)], dtype=np.uint8)


def encode(L, rate: int, base: int, frame: np.ndarray) -> np.ndarray:
    n = L.turboref_codeword_length(rate, base)
    bits = np.zeros(n, np.uint8)
    fr = np.ascontiguousarray(frame)
    L.turboref_encode(rate, base, fr.ctypes.data, bits.ctypes.data)
    assert bits.max() <= 1
    return bits


def wire_frame(L, rate: int, base: int, frame: np.ndarray, flip=None) -> np.ndarray:
    """ASM + the randomised codeword, as bits"""
    cw = encode(L, rate, base, frame)
    if flip is not None:
        cw = cw.copy()
        cw[flip] ^= 1
    return np.concatenate([asm_bits(rate), cw ^ np.resize(soft_pn(), len(cw))])


def quantise(v: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(v), -127, 127).astype(np.int8)


def run_module(L, p: dict, soft: np.ndarray, cuts=(), iters=None, extras=False) -> dict:
    h = L.turboref_create(RATES[p["turbo_rate"]], p["turbo_base"], p["turbo_iters"] if iters is None else iters)
    soft = np.ascontiguousarray(soft, dtype=np.int8)
    edges = [0] + sorted(c for c in cuts if 0 < c < len(soft)) + [len(soft)]
    for a, b in zip(edges[:-1], edges[1:]):
        piece = np.ascontiguousarray(soft[a:b])
        L.turboref_feed(h, piece.ctypes.data, len(piece))
    nd, no = L.turboref_ndesc(h), L.turboref_nout(h)
    r = dict(offset=np.zeros(nd, np.int64), pos=np.zeros(nd, np.int32), swapped=np.zeros(nd, np.int32), cor=np.zeros(nd, np.float32), crc_ok=np.zeros(nd, np.int32),
             out=np.zeros(no, np.uint8), stats=np.zeros(3, np.int32), stat_cor=np.zeros(1, np.float32))
    L.turboref_results(h, *[r[k].ctypes.data for k in ("offset", "pos", "swapped", "cor", "crc_ok", "out", "stats", "stat_cor")])
    if extras:
        F = L.turboref_frame_size(h)
        A = len(ASM_HEX[RATES[p["turbo_rate"]]]) * 4
        a = np.zeros(A, np.float32)
        L.turboref_asm(h, a.ctypes.data)
        r["asm"] = a
        head = np.ascontiguousarray(soft[: 2 * F])
        r["pos_cor"] = np.zeros(len(head) - A + 1, np.float32)
        L.turboref_positions(h, head.ctypes.data, len(head), r["pos_cor"].ctypes.data)
    L.turboref_destroy(h)
    return r


def same(a: dict, b: dict) -> bool:
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("offset", "pos", "swapped", "cor", "crc_ok", "out", "stats", "stat_cor"))


# Eb/N0 well above the waterfall of each rate: a few per cent hard-decision errors, which the first iteration already removes
AMP = 40.0
SIGMA = {0: 22.0, 1: 30.0, 2: 34.0, 3: 40.0}
NFRAMES = 12
ITERS = {0: 3, 1: 2, 2: 2, 3: 2}


def make_stream(L, rate: int, base: int, rng):
    """Twelve frames. [0] is cut a third in, so the first read finds frame 1's ASM behind its middle (a slide with pos > F / 2). [3] loses five bytes early in
    the frame: its read is in lock and decodes a shifted codeword; the next read starts five bytes into frame 4, where frame 5's ASM lies behind the last position
    the module correlates, so it slides to the greatest sidelobe -- the seed is chosen so that this is a slide with pos <= F / 2, the buffer with the stale
    middle -- and the read after it finds frame 6's ASM. [6] and [7] are inverted. [9] is sent without noise, with one bit of the frame flipped behind its CRC
    (a valid codeword of a frame whose CRC fails). [10]'s codeword is buried in noise (the signal at 0.15 of its amplitude)."""
    n = NFRAMES
    frames = [make_frame(rng, base) for _ in range(n)]
    bad, noisy = 9, 10
    sent = []
    for k, fr in enumerate(frames):
        f2 = fr.copy()
        if k == bad:
            f2[10] ^= 0x04
        sent.append(f2)
    wires = [wire_frame(L, rate, base, f).astype(np.float64) * 2.0 - 1.0 for f in sent]
    F = len(wires[0])
    A = len(ASM_HEX[rate]) * 4
    sig = [np.full(F, SIGMA[rate]) for _ in range(n)]
    sig[bad][:] = 0.0
    sig[noisy][A:] = float(np.hypot(AMP, SIGMA[rate]))
    amp = [np.full(F, AMP) for _ in range(n)]
    amp[noisy][A:] = 0.15 * AMP
    for k in (6, 7):
        wires[k] = -wires[k]
    v = np.concatenate(wires) * np.concatenate(amp) + np.concatenate(sig) * rng.standard_normal(n * F)
    s = quantise(v)
    hard_errors = [int(((s[k * F:(k + 1) * F] > 0) != (wires[k] > 0)).sum()) for k in range(n)]
    lead = F // 3
    drop = 3 * F + 700
    s = np.concatenate([s[lead:drop], s[drop + 5:]])
    return s, frames, dict(lead_cut=lead, dropped=[drop, 5], inverted=[6, 7], crc_bad=bad, noisy=noisy, amp=AMP, sigma=SIGMA[rate], hard_errors=hard_errors), F


EMITTED = [1, 2, 6, 7, 8, 11]


def stream_is_wanted(L, p, s, F) -> bool:
    """the reference's walk over the stream is the one the cases are about (see make_stream)"""
    w = run_module(L, p, s)
    pos = w["pos"]
    return len(pos) == 10 and pos[0] > F // 2 and pos[1] == 0 and pos[2] == 0 and 0 < pos[3] <= F // 2 and pos[4] > 0 and not pos[5:].any() and \
        w["crc_ok"].tolist() == [1, 1, 0, 0, 1, 1, 1, 0, 0, 1]


def save_npz(path: str, arrays: dict):
    """np.savez_compressed with the archive's time stamps pinned: the same arrays give the same file, byte for byte"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue(), compresslevel=9)


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]


def prepared(L, rate: int, base: int, frame: np.ndarray, sigma: float, rng) -> np.ndarray:
    """a codeword as CCSDSTurbo::decode receives it: quantised soft bytes * (1 / 127) in float"""
    cw = encode(L, rate, base, frame).astype(np.float64) * 2.0 - 1.0
    q = quantise(cw * AMP + sigma * rng.standard_normal(len(cw)))
    return q.astype(np.float32) * np.float32(1.0 / 127.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "turbo"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    index = ["# produced by tools/gen_ccsds_turbo_golden.py from the reference's own sources (ccsds_turbo_decoder); name, size, key:sha256[:12]"]

    def save(name, arrays):
        path = os.path.join(args.out, name + ".npz")
        save_npz(path, arrays)
        size = os.path.getsize(path)
        assert size <= 512 * 1024, (name, size)
        index.append(f"{name}.npz {size:9d} B  " + " ".join(f"{k}:{sha(v)}" for k, v in sorted(arrays.items())))
        return size

    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(args.ref, tmp)
        base = 223
        for rname, rate in RATES.items():
            p = dict(turbo_rate=rname, turbo_base=base, turbo_iters=ITERS[rate])
            for seed in range(13100 + 100 * rate, 13200 + 100 * rate):  # the first seed whose sidelobe slide is the wanted one
                s, frames, how, F = make_stream(L, rate, base, np.random.default_rng(seed))
                if stream_is_wanted(L, p, s, F):
                    break
            else:
                raise AssertionError(f"{rname}: no seed gives the wanted walk")
            how["seed"] = seed
            n = len(s)
            whole = run_module(L, p, s, extras=True)
            for cuts in ([n // 3, n // 3 + 2345], [1, 7, F - 1, F, F + 1, 3 * F + 11, 3 * F + 12, n - 1], list(range(777, n, 5003))):
                assert same(whole, run_module(L, p, s, cuts=cuts)), f"{rname}: the restated loop's output DEPENDS on how the input is cut ({cuts[:3]}...)"
            fewer = run_module(L, p, s, iters=ITERS[rate] - 1)
            assert np.array_equal(fewer["out"], whole["out"]) and np.array_equal(fewer["crc_ok"], whole["crc_ok"]), f"{rname}: the output changes with the last iteration"
            got = whole["out"].reshape(-1, base + 4)
            assert (got[:, :4] == np.array([0x1A, 0xCF, 0xFC, 0x1D], np.uint8)).all()
            sent = {f.tobytes(): k for k, f in enumerate(frames)}
            ids = [sent.get(g[4:].tobytes(), -1) for g in got]
            assert all(i >= 0 for i in ids) and ids == sorted(set(ids)), ids
            assert len(ids) * 2 >= len(frames), (rname, ids)
            assert ids == EMITTED, ids
            assert all(how["hard_errors"][i] >= 20 for i in ids), how["hard_errors"]  # every emitted frame was corrected
            pos, sw = whole["pos"], whole["swapped"]
            assert pos[0] > F // 2, pos[:2]
            assert ((pos > 0) & (pos <= F // 2)).any(), pos
            small = np.flatnonzero((pos > 0) & (pos <= F // 2))
            assert not whole["crc_ok"][small].any()
            assert sw.any() and not sw.all()
            assert whole["crc_ok"][sw != 0].sum() >= 2
            arrays = dict(soft=s, params=np.frombuffer(json.dumps(dict(p, how=how, F=F)).encode(), dtype=np.uint8), **whole)
            # the stream cut inside the FIRST slide's extra read (the start mid-frame): the module has its correlation, the buffer is not decoded yet
            tl = F + int(pos[0]) // 2
            t = run_module(L, p, s[:tl])
            assert len(t["offset"]) == 0 and t["stats"][0] == 0 and t["stats"][2] == 1
            # ... and inside the second one's
            k = int(small[0])
            tl2 = int(whole["offset"][k]) + F + max(1, int(pos[k]) // 2)
            t2 = run_module(L, p, s[:tl2])
            assert len(t2["offset"]) == k and t2["stats"][0] == 0 and t2["stats"][2] == 1
            arrays.update(trunc_len=np.array([tl, tl2], np.int64), trunc_stats=np.stack([t["stats"], t2["stats"]]), trunc_cor=np.concatenate([t["stat_cor"], t2["stat_cor"]]),
                          trunc_reads=np.array([0, k], np.int32))
            size = save("r" + rname.replace("/", "") + "_b223", arrays)
            print(f"r{rname}: F {F}, {len(pos)} buffers, pos {pos.tolist()}, swapped {sw.tolist()}, crc_ok {whole['crc_ok'].tolist()}, frames {ids}, {size} B; "
                  f"three cuttings and one iteration fewer leave the output unchanged")
        # ---- unit
        arrays = {}
        for b in (223, 446, 892, 1115):
            pi = np.zeros(b * 8, np.int32)
            L.turboref_pi(b, pi.ctypes.data)
            assert sorted(pi.tolist()) == list(range(b * 8))
            arrays[f"pi_{b}"] = pi.astype(np.uint16)
        rng = np.random.default_rng(13200)
        for rname in ("1/2", "1/6"):
            rate = RATES[rname]
            tag = "bcjr_r" + rname.replace("/", "")
            Lb = 223 * 8
            nu, nl = [(2, 1), (2, 1), (3, 1), (4, 2)][rate]
            cw = prepared(L, rate, 223, make_frame(rng, 223), SIGMA[rate] * 1.5, rng)
            s0, s1 = np.zeros(nu * (Lb + 4)), np.zeros(nl * (Lb + 4))
            au, li, al = np.zeros((2, Lb)), np.zeros((2, Lb)), np.zeros((2, Lb))
            L.turboref_bcjr(rate, 223, cw.ctypes.data, s0.ctypes.data, s1.ctypes.data, au.ctypes.data, li.ctypes.data, al.ctypes.data)
            assert np.isfinite(au).all() and np.isfinite(al).all() and not np.array_equal(au, al)
            arrays.update({tag + "_cw": cw, tag + "_stream0": s0, tag + "_stream1": s1, tag + "_after_upper": au, tag + "_lower_in": li, tag + "_after_lower": al})
        for b, rname in ((446, "1/3"), (892, "1/4"), (1115, "1/6")):
            rate = RATES[rname]
            tag = f"dec_b{b}_r" + rname.replace("/", "")
            frs = [make_frame(rng, b) for _ in range(2)]
            cws = np.stack([prepared(L, rate, b, f, SIGMA[rate] * sc, rng) for f, sc in zip(frs, (1.0, 1.6))])
            arrays[tag + "_cw"] = (np.rint(cws.astype(np.float64) * 127.0)).astype(np.int8)  # (stored as the soft bytes: cw = byte * (1 / 127) in float32)
            assert np.array_equal(arrays[tag + "_cw"].astype(np.float32) * np.float32(1.0 / 127.0), cws)
            arrays[tag + "_sent"] = np.stack([np.unpackbits(f) for f in frs])
            for it in (1, 2):
                bits = np.zeros((2, b * 8), np.uint8)
                L.turboref_decode(rate, b, it, cws.ctypes.data, 2, bits.ctypes.data)
                arrays[f"{tag}_bits_{it}"] = np.packbits(bits, axis=1)
            ok = [bool(np.array_equal(np.unpackbits(arrays[f"{tag}_bits_2"][k]), arrays[tag + "_sent"][k])) for k in range(2)]
            assert ok[0], tag
            print(f"{tag}: decoded to the transmitted frame after 2 iterations: {ok}")
        rcw = np.clip(np.rint((encode(L, 1, 223, make_frame(rng, 223)).astype(np.float64) * 2.0 - 1.0) * 100.0 + 40.0 * rng.standard_normal(5364)), -128, 127).astype(np.int8)
        assert (rcw == -128).sum() >= 20 and (rcw == 127).sum() >= 20
        rf = rcw.astype(np.float32) * np.float32(1.0 / 127.0)
        rb = np.zeros((1, 223 * 8), np.uint8)
        L.turboref_decode(1, 223, 2, rf.ctypes.data, 1, rb.ctypes.data)
        arrays.update(rails_cw=rcw[None, :], rails_bits_2=np.packbits(rb, axis=1))
        size = save("turbo_unit", arrays)
        print(f"turbo_unit: {size} B")
    with open(os.path.join(args.out, "INDEX.txt"), "w") as f:
        f.write("\n".join(index) + "\n")


if __name__ == "__main__":
    main()
