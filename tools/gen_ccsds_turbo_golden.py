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
and at least half of the frames sent are emitted; the output is the same for three cuttings of each stream.

INSIDE THE WATERFALL (all of the above lies well above it: one iteration decodes it). The driver's turboref_iterate runs turbo_decode's loop by hand over
convcode_extrinsic and returns the decided bits after every iteration (asserted equal to CCSDSTurbo::decode's for every iteration count recorded) and, on request,
the a-priori arrays into and out of each constituent pass. With its perturbation option every message m becomes m + s 2^-43 max(1, |m|) after every pass (s = +-1,
seeded); a (frame, iteration) pair is STABLE when two differently seeded perturbed runs both give the unperturbed bits. Sigma and seed are searched until: iterations
1 and 2 of every frame are stable, every iteration from a frame's first clean one onwards is stable, and at least 90 % of all recorded pairs are (reached: 232 of 232).
    turbo_iter_r12 / r13 / r14 / r16.npz   base 223: soft [5][n] (soft bytes), sent (the frames), bits [5][8][base] (packed, after k = 1 .. 8 iterations), stable [5][8],
                              first [5] (the first clean iteration, 0 = never in 8: at least three in 3 .. 8 and at least one 0), and for frame pass_frame at the
                              iterations pass_iters (the one before its first clean one, and 8, whose arrays must hold |m| > 40): passes [2][4][2][L], the a-priori
                              arrays the upper pass receives and leaves and the lower pass receives (interleaved) and leaves, with stream0 / stream1
    turbo_combos_a / _b.npz   one codeword for each rate with each of the bases 446, 892, 1115, first clean at an iteration in 3 .. 6: r12_b446_soft, _sent, _bits [6][base],
                              _stable [6], _first (a: rates 1/2, 1/3, 1/4; b: rate 1/6)
    unlocked_r12 / r16_b223.npz   ten reads of noise only, every one a slide, two thirds of a read more, three frames at SIGMA, half a read of noise; the stream files'
                              fields. Asserted: the first eleven reads slide, the eleventh with pos > F / 2 onto the first frame, lock follows, the three frames are emitted
    r13_b446, r14_b892, r12_b1115.npz   five frames at turbo_iters = 5: a start mid-frame, [2] inverted, [3] buried in noise, the others inside the waterfall (their bits
                              stable after 3 and after 5 iterations); the stream files' fields and out_fewer, crc_ok_fewer: what the module emits at turbo_iters - 2,
                              asserted a non-empty strict subset. A base 1115 rate 1/6 stream of five frames would not fit the 512 KiB a file may take: left out."""
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
    L.turboref_iterate.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_uint64]
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


# ---- inside the waterfall -------------------------------------------------------------------------------------------------------------------------------
K_ITER, K_COMBO = 8, 6
# noise at which a frame needs several iterations, and some frames never decode (AMP = 40); the search below walks seeds (and these sigmas) until its conditions hold
WATERFALL = {0: [35.0, 34.0, 36.0], 1: [47.0, 46.0, 48.0], 2: [58.0, 57.0, 59.0], 3: [68.0, 67.0, 69.0]}
# the longer blocks take more iterations at the same noise: a little less of it brings the first clean iteration into 3 .. 6
LONGER = {r: [round(w[0] * f, 1) for f in (0.93, 0.89, 0.97)] for r, w in WATERFALL.items()}
COMPONENTS = [(2, 1), (2, 1), (3, 1), (4, 2)]
PERTURB = (0x5EED0001, 0x5EED0002)
STREAM_KEYS = ("offset", "pos", "swapped", "cor", "crc_ok", "out", "stats", "stat_cor")


def soft_codeword(L, rate: int, base: int, frame: np.ndarray, sigma: float, rng) -> np.ndarray:
    cw = encode(L, rate, base, frame).astype(np.float64) * 2.0 - 1.0
    return quantise(cw * AMP + sigma * rng.standard_normal(len(cw)))


def as_prepared(q: np.ndarray) -> np.ndarray:
    return q.astype(np.float32) * np.float32(1.0 / 127.0)


def iterate(L, rate: int, base: int, cw: np.ndarray, iters: int, rec=None, perturb: int = 0):
    """turbo_decode's loop by hand (turboref_iterate): bits [iters][L], the recorded passes [2][4][2][L] of the iterations `rec`, the two constituent streams"""
    Lb = base * 8
    nu, nl = COMPONENTS[rate]
    cw = np.ascontiguousarray(cw, dtype=np.float32)
    assert len(cw) == L.turboref_codeword_length(rate, base)
    bits = np.zeros((iters, Lb), np.uint8)
    r = np.array(rec if rec else [0, 0], np.int32)
    passes = np.zeros((2, 4, 2, Lb)) if rec else None
    s0, s1 = np.zeros(nu * (Lb + 4)), np.zeros(nl * (Lb + 4))
    L.turboref_iterate(rate, base, cw.ctypes.data, iters, bits.ctypes.data, r.ctypes.data, passes.ctypes.data if rec else None, s0.ctypes.data, s1.ctypes.data, perturb)
    return bits, passes, s0, s1


def first_clean(bits: np.ndarray, sent: np.ndarray) -> int:
    clean = (bits == sent[None, :]).all(1)
    return int(np.argmax(clean)) + 1 if clean.any() else 0


def stable_mask(L, rate: int, base: int, cw: np.ndarray, bits: np.ndarray) -> np.ndarray:
    """stable[k - 1]: two differently seeded perturbed runs both give the unperturbed bits after k iterations"""
    st = np.ones(len(bits), bool)
    for seed in PERTURB:
        st &= (iterate(L, rate, base, cw, len(bits), perturb=seed)[0] == bits).all(1)
    return st


def holds(first: int, st: np.ndarray) -> bool:
    """the two conditions no search may give up: iterations 1 and 2 are stable, and so is every iteration from the first clean one onwards"""
    return bool(st[:2].all() and (first == 0 or st[first - 1:].all()))


def is_turbo_decode(L, rate: int, base: int, cw: np.ndarray, bits: np.ndarray):
    """the hand loop's bits are CCSDSTurbo::decode's, for every iteration count recorded"""
    cw = np.ascontiguousarray(cw, dtype=np.float32)
    for k in range(1, len(bits) + 1):
        b = np.zeros((1, base * 8), np.uint8)
        L.turboref_decode(rate, base, k, cw.ctypes.data, 1, b.ctypes.data)
        assert np.array_equal(b[0], bits[k - 1]), (rate, base, k)


def make_iter_fixture(L, rate: int, rname: str):
    """five base 223 codewords inside the waterfall: at least three first clean at an iteration in 3 .. 8, at least one never clean in K_ITER"""
    base, Lb = 223, 223 * 8
    best = None
    for sigma in WATERFALL[rate]:
        for seed in range(13300 + 100 * rate, 13400 + 100 * rate):
            rng = np.random.default_rng(seed)
            got, nconv, nnever = [], 0, 0
            for _ in range(24):
                fr = make_frame(rng, base)
                q = soft_codeword(L, rate, base, fr, sigma, rng)
                sent = np.unpackbits(fr)
                bits = iterate(L, rate, base, as_prepared(q), K_ITER)[0]
                first = first_clean(bits, sent)
                if not ((3 <= first <= K_ITER and nconv < 4) or (first == 0 and nnever < 2)):
                    continue
                st = stable_mask(L, rate, base, as_prepared(q), bits)
                if not holds(first, st):
                    continue
                nconv, nnever = nconv + (first != 0), nnever + (first == 0)
                got.append((fr, q, bits, first, st))
                if len(got) == 5:
                    break
            if len(got) < 5:
                continue
            share = float(np.mean([g[4] for g in got]))
            # the frame whose passes are recorded: a converging one whose a-priori values in K_ITER hold |m| > 40 (beyond exp_sum's log(1 + exp(-40)) == 0)
            pf = [k for k, g in enumerate(got) if g[3] >= 3 and (np.abs(iterate(L, rate, base, as_prepared(g[1]), K_ITER, rec=[g[3] - 1, K_ITER])[1][1]) > 40.0).any()]
            if not pf:
                continue
            if best is None or share > best[0]:
                best = (share, sigma, seed, got, pf[0])
            if share >= 0.9:
                break
        if best is not None and best[0] >= 0.9:
            break
    assert best is not None, f"{rname}: no seed gives five codewords of the wanted kinds"
    share, sigma, seed, got, pf = best
    firsts = [g[3] for g in got]
    assert sum(3 <= f <= K_ITER for f in firsts) >= 3 and firsts.count(0) >= 1, firsts
    for fr, q, bits, first, st in got:
        assert holds(first, st)
        is_turbo_decode(L, rate, base, as_prepared(q), bits)
    rec = [firsts[pf] - 1, K_ITER]  # the iteration before the first clean one, and the last
    bits, passes, s0, s1 = iterate(L, rate, base, as_prepared(got[pf][1]), K_ITER, rec=rec)
    assert np.array_equal(bits, got[pf][2]) and np.isfinite(passes).all()
    assert (np.abs(passes[1]) > 40.0).any(), "the passes of the last iteration hold no |m| > 40"
    pi = np.zeros(Lb, np.int32)
    L.turboref_pi(base, pi.ctypes.data)
    for x in range(2):
        assert np.array_equal(passes[x, 2], passes[x, 1][:, pi])  # the lower pass receives message_interleave of what the upper one left
    how = dict(turbo_rate=rname, turbo_base=base, amp=AMP, sigma=sigma, seed=seed, stable_share=share, first_clean=firsts, perturb=list(PERTURB))
    arrays = dict(soft=np.stack([g[1] for g in got]), sent=np.stack([g[0] for g in got]), bits=np.stack([np.packbits(g[2], axis=1) for g in got]),
                  stable=np.stack([g[4] for g in got]).astype(np.uint8), first=np.array(firsts, np.int32), pass_frame=np.array([pf], np.int32), pass_iters=np.array(rec, np.int32),
                  passes=passes, stream0=s0, stream1=s1, params=np.frombuffer(json.dumps(how).encode(), dtype=np.uint8))
    return arrays, how


def make_combo(L, rate: int, base: int, seed0: int):
    """one codeword of (rate, base) first clean at an iteration in 3 .. K_COMBO, with the two conditions of holds()"""
    for sigma in LONGER[rate]:
        for seed in range(seed0, seed0 + 100):
            rng = np.random.default_rng(seed)
            fr = make_frame(rng, base)
            q = soft_codeword(L, rate, base, fr, sigma, rng)
            bits = iterate(L, rate, base, as_prepared(q), K_COMBO)[0]
            first = first_clean(bits, np.unpackbits(fr))
            if not 3 <= first <= K_COMBO:
                continue
            st = stable_mask(L, rate, base, as_prepared(q), bits)
            if holds(first, st):
                is_turbo_decode(L, rate, base, as_prepared(q), bits)
                return dict(soft=q, sent=fr, bits=np.packbits(bits, axis=1), stable=st.astype(np.uint8), first=np.array([first], np.int32)), dict(sigma=sigma, seed=seed, first_clean=first)
    raise AssertionError(f"rate {rate} base {base}: no seed gives a codeword first clean in 3 .. {K_COMBO}")


def stream_arrays(L, p: dict, s: np.ndarray, F: int, how: dict, second: int) -> dict:
    """a stream fixture's fields: the whole run (asserted the same for three cuttings), and the statistics inside the first slide's extra read and inside read `second`'s"""
    n = len(s)
    whole = run_module(L, p, s, extras=True)
    for cuts in ([n // 3, n // 3 + 2345], [1, 7, F - 1, F, F + 1, 3 * F + 11, 3 * F + 12, n - 1], list(range(777, n, 5003))):
        assert same(whole, run_module(L, p, s, cuts=cuts)), f"{p}: the restated loop's output DEPENDS on how the input is cut ({cuts[:3]}...)"
    pos = whole["pos"]
    assert pos[0] != 0 and pos[second] != 0
    tl = F + max(1, int(pos[0]) // 2)
    t = run_module(L, p, s[:tl])
    assert len(t["offset"]) == 0 and t["stats"][0] == 0 and t["stats"][2] == 1
    tl2 = int(whole["offset"][second]) + F + max(1, int(pos[second]) // 2)
    t2 = run_module(L, p, s[:tl2])
    assert len(t2["offset"]) == second and t2["stats"][0] == 0 and t2["stats"][2] == 1
    return dict(soft=s, params=np.frombuffer(json.dumps(dict(p, how=how, F=F)).encode(), dtype=np.uint8), **whole, trunc_len=np.array([tl, tl2], np.int64),
                trunc_stats=np.stack([t["stats"], t2["stats"]]), trunc_cor=np.concatenate([t["stat_cor"], t2["stat_cor"]]), trunc_reads=np.array([0, second], np.int32))


def emitted_ids(out: np.ndarray, base: int, frames) -> list:
    got = out.reshape(-1, base + 4)
    assert (got[:, :4] == np.array([0x1A, 0xCF, 0xFC, 0x1D], np.uint8)).all()
    sent = {f.tobytes(): k for k, f in enumerate(frames)}
    return [sent.get(g[4:].tobytes(), -1) for g in got]


def make_unlocked(L, rate: int, rname: str):
    """ten reads of noise only (every one slides: the serial walk), two thirds of a read more, three frames at SIGMA, half a read of noise"""
    base = 223
    p = dict(turbo_rate=rname, turbo_base=base, turbo_iters=ITERS[rate])
    level = float(np.hypot(AMP, SIGMA[rate]))
    for seed in range(13700 + 100 * rate, 13800 + 100 * rate):
        rng = np.random.default_rng(seed)
        frames = [make_frame(rng, base) for _ in range(3)]
        wires = [wire_frame(L, rate, base, f).astype(np.float64) * 2.0 - 1.0 for f in frames]
        F = len(wires[0])
        noise = quantise(level * rng.standard_normal(24 * F))
        sig = quantise(np.concatenate(wires) * AMP + SIGMA[rate] * rng.standard_normal(3 * F))
        tail = quantise(level * rng.standard_normal(F // 2))
        w = run_module(L, p, noise)
        if len(w["pos"]) < 10 or not w["pos"][:10].all():
            continue
        lead = int(w["offset"][9]) + F + int(w["pos"][9]) + 2 * F // 3  # behind the tenth read: the eleventh finds frame 0's ASM behind its middle
        s = np.concatenate([noise[:lead], sig, tail])
        w = run_module(L, p, s)
        pos = w["pos"]
        if not (len(pos) == 13 and pos[:11].all() and pos[10] > F // 2 and not pos[11:].any() and w["crc_ok"][10:].all()):
            continue
        assert emitted_ids(w["out"], base, frames)[-3:] == [0, 1, 2]
        assert not w["crc_ok"][:10].any() and w["stats"][0] == 1
        how = dict(seed=seed, lead=lead, noise_reads=10, amp=AMP, sigma=SIGMA[rate], noise=level)
        return stream_arrays(L, p, s, F, how, 1), pos
    raise AssertionError(f"{rname}: no seed gives ten sliding reads and then lock")


def make_long_stream(L, rate: int, rname: str, base: int, seed0: int):
    """five frames, turbo_iters = 5: [0] is cut a third in (a slide with pos > F / 2), [2] is inverted, [3]'s codeword is buried in noise, the others lie inside the
    waterfall. At least one frame is first clean at iteration 4 or 5, so the frames emitted at turbo_iters - 2 are a strict subset; the bits of every frame sent
    inside the waterfall are stable (see stable_mask) after 3 and after 5 iterations, where the CRC gate looks at them."""
    iters = 5
    p = dict(turbo_rate=rname, turbo_base=base, turbo_iters=iters)
    A = len(ASM_HEX[rate]) * 4
    pn = None
    for sigma in LONGER[rate]:
        for seed in range(seed0, seed0 + 100):
            rng = np.random.default_rng(seed)
            frames = [make_frame(rng, base) for _ in range(5)]
            wires = [wire_frame(L, rate, base, f).astype(np.float64) * 2.0 - 1.0 for f in frames]
            F = len(wires[0])
            if pn is None:
                pn = np.resize(soft_pn(), F - A).astype(bool)
            wires[2] = -wires[2]
            sig = [np.full(F, sigma) for _ in range(5)]
            amp = [np.full(F, AMP) for _ in range(5)]
            sig[3][A:] = float(np.hypot(AMP, sigma))
            amp[3][A:] = 0.15 * AMP
            full = quantise(np.concatenate(wires) * np.concatenate(amp) + np.concatenate(sig) * rng.standard_normal(5 * F))
            firsts, ok = {}, True
            for k in (1, 2, 4):
                seg = full[k * F + A:(k + 1) * F]
                cw = as_prepared(np.where(pn, ~seg, seg))  # derand_ccsds_soft is ~x
                cw = -cw if k == 2 else cw
                bits = iterate(L, rate, base, cw, iters)[0]
                firsts[k] = first_clean(bits, np.unpackbits(frames[k]))
                st = stable_mask(L, rate, base, cw, bits)
                ok = ok and holds(firsts[k], st) and bool(st[iters - 3] and st[iters - 1])
            f = list(firsts.values())
            if not (ok and any(1 <= x <= iters - 2 for x in f) and any(iters - 2 < x <= iters for x in f)):
                continue
            s = full[F // 3:]
            w = run_module(L, p, s)
            fewer = run_module(L, p, s, iters=iters - 2)
            ids, ids_fewer = emitted_ids(w["out"], base, frames), emitted_ids(fewer["out"], base, frames)
            want = [k for k in (1, 2, 4) if 1 <= firsts[k] <= iters]
            if not (len(w["pos"]) == 4 and w["pos"][0] > F // 2 and not w["pos"][1:].any() and w["swapped"].tolist() == [0, 1, 0, 0] and ids == want):
                continue
            assert ids_fewer == [k for k in (1, 2, 4) if 1 <= firsts[k] <= iters - 2] and 0 < len(ids_fewer) < len(ids), (ids, ids_fewer)
            assert set(ids_fewer) < set(ids) and not w["crc_ok"][2]
            for k in ("offset", "pos", "swapped", "cor"):
                assert np.array_equal(w[k], fewer[k])
            how = dict(seed=seed, lead_cut=F // 3, inverted=[2], noisy=3, amp=AMP, sigma=sigma, first_clean=[firsts[k] for k in (1, 2, 4)], emitted=ids, emitted_fewer=ids_fewer)
            arrays = stream_arrays(L, p, s, F, how, 0)
            arrays.update(out_fewer=fewer["out"], crc_ok_fewer=fewer["crc_ok"])
            return arrays, how
    raise AssertionError(f"{rname} base {base}: no seed gives a stream that needs its iterations")


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
        # ---- inside the waterfall (new files only: nothing above draws from these generators)
        shares = []
        for rname, rate in RATES.items():
            arrays, how = make_iter_fixture(L, rate, rname)
            shares += arrays["stable"].ravel().tolist()
            size = save("turbo_iter_r" + rname.replace("/", ""), arrays)
            print(f"turbo_iter r{rname}: sigma {how['sigma']}, seed {how['seed']}, first clean {how['first_clean']}, stable {how['stable_share']:.3f}, passes of frame "
                  f"{int(arrays['pass_frame'][0])} at {arrays['pass_iters'].tolist()}, max |m| {np.abs(arrays['passes'][1]).max():.1f}, {size} B")
        combos = {"a": {}, "b": {}}
        for rname, rate in RATES.items():
            for b in (446, 892, 1115):
                arrays, how = make_combo(L, rate, b, 14000 + 1000 * rate + b)
                shares += arrays["stable"].ravel().tolist()
                tag = f"r{rname.replace('/', '')}_b{b}"
                combos["b" if rate == 3 else "a"].update({f"{tag}_{k}": v for k, v in arrays.items()})
                print(f"turbo_combos {tag}: {how}, stable {arrays['stable'].tolist()}")
        for half, arrays in combos.items():
            print(f"turbo_combos_{half}: {save('turbo_combos_' + half, arrays)} B")
        share = float(np.mean(shares))
        print(f"stable (frame, iteration) pairs: {int(np.sum(shares))} of {len(shares)} ({share:.4f})")
        assert share >= 0.9, share
        for rname in ("1/2", "1/6"):
            arrays, pos = make_unlocked(L, RATES[rname], rname)
            size = save("unlocked_r" + rname.replace("/", "") + "_b223", arrays)
            print(f"unlocked r{rname}: pos {pos.tolist()}, crc_ok {arrays['crc_ok'].tolist()}, {size} B")
        for rname, b in (("1/3", 446), ("1/4", 892), ("1/2", 1115)):
            arrays, how = make_long_stream(L, RATES[rname], rname, b, 15000 + b)
            size = save(f"r{rname.replace('/', '')}_b{b}", arrays)
            print(f"r{rname} base {b}: {how}, pos {arrays['pos'].tolist()}, crc_ok {arrays['crc_ok'].tolist()} ({arrays['crc_ok_fewer'].tolist()} at turbo_iters - 2), {size} B")
    with open(os.path.join(args.out, "INDEX.txt"), "w") as f:
        f.write("\n".join(index) + "\n")


if __name__ == "__main__":
    main()
