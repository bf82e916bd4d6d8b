#!/usr/bin/env python3
"""tools/gen_ccsds_ldpc_golden.py -- records what the reference's ccsds_ldpc_decoder computes at "ldpc_rate": "7/8" as fixtures under tests/golden/ldpc/.

Needs the reference tree (REF, default /root/reference) and g++; the tests that read the fixtures need neither. The driver tools/ccsds_ldpc_golden_driver.cpp is
compiled with the reference's own sources (CorrelatorGeneric, CCSDSLDPC over LDPCDecoderGeneric, rotate_soft, derand_ccsds_soft, BPSK_CCSDS_Deframer), included
and compiled where they lie, into a TEMPORARY directory with the oracle's recorded flags (-O2 -ffp-contract=off, ref_shim/); nothing compiled stays behind.

The streams are built here: codewords of the (8176, 7154) code from a GF(2) elimination of its parity check matrix (every word is checked against H), the wire
format around them (ASM, randomiser, two fill bits, the constellation's bit-to-soft mapping, AWGN) and the damage each case is about. tests/golden/ldpc/INDEX.txt
lists the files. Every stream file holds
    soft                      the input (int8)
    params                    JSON: the module's keys and how the stream was made
    offset, sync, cor, corrections, locked      one entry per frame the module decoded (stream position of its first byte, CorrelatorGeneric's best_sync, ...)
    out                       the bytes the module writes (frames of 1024 bytes, or CADUs)
    frames                    (internal_stream only) what the direct branch writes for the same stream
    trunc_len, trunc_stats, trunc_cor   (streams with a slide) the statistics behind the stream's first trunc_len bytes, which end inside a slide's extra read
    stats                     int32 {correlator_lock, ldpc_corr, deframer state, 0}; stat_cor float32 correlator_corr
    syncwords                 the correlator's tables, float32 [n][32]
    pos_cor, pos_sync         per position of the first 4 frames' bytes: the correlation and syncword CorrelatorGeneric::correlate reports for that position alone
r78_unit.npz holds 16 prepared codewords at three noise levels and, for 1, 10 and 25 iterations, the packed hard bits and CCSDSLDPC::decode's return values; the
code's row list; and `g_*`: a small irregular code (check nodes of 3 .. 9 edges, odd degrees among them), words for it, and LDPCDecoderGeneric's bits and return
values on that row list after 1 and 6 iterations.

r78_rails.npz, r78_rails_oqpsk.npz and r78_rails_bpsk.npz are streams quantised to the WHOLE int8 range at an amplitude that saturates (12 QPSK frames in the four
turns, 4 OQPSK frames of the two Q-shifted tables, 4 BPSK frames with the second half inverted): -128 in front of rotate_soft, and, where the stream is derandomised,
127s that the soft derandomiser turns into -128 in front of the decoder. r78_rails.npz also holds `rails_*`: 8 prepared codewords with -128 among them and
CCSDSLDPC::decode's bits and return values on them after 1 and 10 iterations.

The generator asserts, and fails otherwise: in every rails stream at least 2 % of the bytes are -128 and at least 2 % are 127, and at least 8 of r78_rails' 12 frames
are corrected to the transmitted word; the output is the same for three cuttings of each stream; in r78_qpsk_direct and r78_oqpsk_internal at least half of the
frames have corrections > 0 and decode to the transmitted word; every noisy case has a frame that does not; in r78_unit a word is right after 10 iterations and
wrong after 1; every syncword index of each constellation occurs in some descriptor."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CPP = ["common/codings/generic_correlator.cpp", "common/codings/rotation.cpp", "common/codings/randomization.cpp", "common/codings/deframing/bpsk_ccsds_deframer.cpp",
           "common/codings/ldpc/ccsds_ldpc.cpp", "common/codings/ldpc/ldpc_decoder_generic.cpp", "common/codings/ldpc/make_ccsds.cpp",
           "common/codings/ldpc/matrix/matrix.cpp", "common/codings/ldpc/matrix/sparse_matrix.cpp"]
F, CW, N, M, LEAD, DATA = 8192, 8160, 8176, 1022, 18, 7136
BPSK, QPSK, OQPSK = 0, 2, 3  # SDHIP_BPSK / SDHIP_QPSK / SDHIP_OQPSK
ASM = 0x1ACFFC1D
# first-row positions of the sixteen weight-two circulants in each of the two block rows (CCSDS 131.1-O-2, the (8176, 7154) code)
CIRC = [[(0, 176), (12, 239), (0, 352), (24, 431), (0, 392), (151, 409), (0, 351), (9, 359), (0, 307), (53, 329), (0, 207), (18, 281), (0, 399), (202, 457), (0, 247), (36, 261)],
        [(99, 471), (130, 473), (198, 435), (260, 478), (215, 420), (282, 481), (48, 396), (193, 445), (273, 430), (302, 451), (96, 379), (191, 386), (244, 467), (364, 470),
         (51, 382), (192, 414)]]


def parity_check_matrix() -> np.ndarray:
    H = np.zeros((M, N), dtype=np.uint8)
    for by in range(2):
        for r in range(511):
            for bx in range(16):
                for c in CIRC[by][bx]:
                    H[by * 511 + r, 511 * bx + (c + r) % 511] = 1
    assert (H.sum(1) == 32).all() and (H.sum(0) == 4).all()
    return H


class Encoder:
    """Reduced row echelon form of H with the pivots taken from the right: the pivot columns are parity, every other column is free."""

    def __init__(self):
        self.H = parity_check_matrix()
        A = self.H.copy()
        piv, r = [], 0
        for c in range(N - 1, -1, -1):
            if r == M:
                break
            rows = np.flatnonzero(A[r:, c]) + r
            if len(rows) == 0:
                continue
            if rows[0] != r:
                A[[r, rows[0]]] = A[[rows[0], r]]
            others = np.flatnonzero(A[:, c])
            others = others[others != r]
            A[others] ^= A[r]
            piv.append(c)
            r += 1
        self.rank = r
        self.piv = np.array(piv)
        self.A = A[:r]
        self.Ad = self.A[:, :LEAD + DATA].astype(np.float32)  # (sums stay below 2^24: exact)
        self.Hf = self.H.astype(np.float32)
        assert self.rank == 1020 and self.piv.min() >= LEAD + DATA, (self.rank, self.piv.min())  # the 7136 data positions (and the 18 in front) are free

    def encode(self, data: np.ndarray) -> np.ndarray:
        """data: 7136 bits -> the 8176-bit word with word[18:7154] = data, word[:18] = 0 and the free parity positions 0"""
        w = np.zeros(N, dtype=np.uint8)
        w[LEAD:LEAD + DATA] = data
        w[self.piv] = (self.Ad @ w[:LEAD + DATA].astype(np.float32)).astype(np.int64) & 1
        assert not ((self.Hf @ w.astype(np.float32)).astype(np.int64) & 1).any()
        return w


def soft_pn() -> np.ndarray:
    reg, out = 0xFF, []
    for _ in range(255):
        out.append(reg & 1)
        fb = (reg ^ (reg >> 3) ^ (reg >> 5) ^ (reg >> 7)) & 1
        reg = (reg >> 1) | (fb << 7)
    return np.array(out, dtype=np.uint8)


def wire_frame(word: np.ndarray, derand: bool) -> np.ndarray:
    """ASM + the shortened word + two fill bits, randomised behind the ASM: 8192 bits"""
    cw = np.concatenate([word[LEAD:], np.zeros(2, dtype=np.uint8)])
    if derand:
        cw = cw ^ np.resize(soft_pn(), CW)
    asm = np.array([(ASM >> (31 - i)) & 1 for i in range(32)], dtype=np.uint8)
    return np.concatenate([asm, cw])


def packed_frame(word: np.ndarray) -> bytes:
    return np.packbits(np.concatenate([word[LEAD:], np.zeros(2, dtype=np.uint8)])).tobytes()


def quantise(v: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(v), -127, 127).astype(np.int8)


def build_driver(ref: str, tmp: str) -> C.CDLL:
    sc = os.path.join(ref, "src-core")
    flags = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-DSOURCE_PATH_SIZE=0", "-I" + os.path.join(ROOT, "ref_shim"), "-I" + sc, "-w", "-fno-access-control",
             "-Dvolk_8i_s32f_convert_32f=volk_8i_s32f_convert_32f_u"]
    lib = os.path.join(tmp, "libldpcref.so")
    subprocess.check_call(["g++"] + flags + ["-shared", "-o", lib, os.path.join(ROOT, "tools", "ccsds_ldpc_golden_driver.cpp")] + [os.path.join(sc, f) for f in REF_CPP] +
                          ["-lpthread", "-lm"])
    L = C.CDLL(lib)
    L.ldpcref_create.restype = C.c_void_p
    L.ldpcref_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32]
    L.ldpcref_destroy.argtypes = [C.c_void_p]
    L.ldpcref_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    for f in ("ldpcref_ndesc", "ldpcref_nout"):
        getattr(L, f).restype = C.c_int64
        getattr(L, f).argtypes = [C.c_void_p]
    L.ldpcref_generic.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.ldpcref_results.argtypes = [C.c_void_p] * 9
    L.ldpcref_syncwords.argtypes = [C.c_void_p, C.c_void_p]
    L.ldpcref_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.ldpcref_unit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L


def run_module(L, p: dict, soft: np.ndarray, cuts=(), internal=None, extras=False) -> dict:
    internal = p["internal_stream"] if internal is None else internal
    h = L.ldpcref_create(p["constellation"], p["derandomize"], p["iterations"], int(internal), p.get("internal_cadu_size", 0), p.get("internal_asm", ASM))
    soft = np.ascontiguousarray(soft, dtype=np.int8)
    edges = [0] + sorted(c for c in cuts if 0 < c < len(soft)) + [len(soft)]
    for a, b in zip(edges[:-1], edges[1:]):
        piece = np.ascontiguousarray(soft[a:b])
        L.ldpcref_feed(h, piece.ctypes.data, len(piece))
    nd, no = L.ldpcref_ndesc(h), L.ldpcref_nout(h)
    r = dict(offset=np.zeros(nd, np.int64), sync=np.zeros(nd, np.int32), cor=np.zeros(nd, np.float32), corrections=np.zeros(nd, np.int32), locked=np.zeros(nd, np.int32),
             out=np.zeros(no, np.uint8), stats=np.zeros(4, np.int32), stat_cor=np.zeros(1, np.float32))
    L.ldpcref_results(h, *[r[k].ctypes.data for k in ("offset", "sync", "cor", "corrections", "locked", "out", "stats", "stat_cor")])
    if extras:
        sw = np.zeros((4, 32), np.float32)
        n = L.ldpcref_syncwords(h, sw.ctypes.data)
        r["syncwords"] = sw[:n].copy()
        head = np.ascontiguousarray(soft[: 4 * F])
        r["pos_cor"] = np.zeros(len(head) - 32, np.float32)
        r["pos_sync"] = np.zeros(len(head) - 32, np.uint8)
        L.ldpcref_positions(h, head.ctypes.data, len(head), r["pos_cor"].ctypes.data, r["pos_sync"].ctypes.data)
    L.ldpcref_destroy(h)
    return r


def same(a: dict, b: dict) -> bool:
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("offset", "sync", "cor", "corrections", "locked", "out", "stats", "stat_cor"))


# ---- the streams ------------------------------------------------------------------------------------------------------------------------------------------
AMP, SIGMA = 48.0, 20.0  # Es/N0 about 4.6 dB per soft bit: some 60 hard-decision errors in a frame, which ten iterations remove


def pairs_stream(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.float64) * 2.0 - 1.0).reshape(-1, 2)


def make_qpsk_direct(enc, rng):
    words = [enc.encode(rng.integers(0, 2, DATA).astype(np.uint8)) for _ in range(32)]
    turns = [0] * 10 + [2] * 6 + [3] * 8 + [1] * 8  # a half turn after frame 9, a QUARTER turn in the middle (frame 16), a half turn after frame 23
    iq = []
    for w, t in zip(words, turns):
        p = pairs_stream(wire_frame(w, True))
        for _ in range(t):
            p = np.stack([-p[:, 1], p[:, 0]], axis=1)
        iq.append(p)
    v = np.concatenate(iq).reshape(-1) * AMP
    sig = np.full(len(v), SIGMA)
    for f in (5, 20):  # two frames buried in noise
        sig[f * F:(f + 1) * F] = 110.0
    v = v + sig * rng.standard_normal(len(v))
    s = quantise(v)
    drop = 12 * F + 4001
    s = np.concatenate([s[3000:drop], s[drop + 5:]])  # the stream starts mid-frame; five bytes dropped once, in lock
    return s, words, dict(turns=turns, noisy=[5, 20], lead_cut=3000, dropped=[drop, 5])


def make_oqpsk_internal(enc, rng):
    # LandSat.json: OQPSK, internal_stream, CADUs of 8272 bits behind the ASM 0x352EF853: 27 CADUs cut into 7136-bit data fields
    asm = np.array([(0x352EF853 >> (31 - i)) & 1 for i in range(32)], dtype=np.uint8)
    stream = np.concatenate([np.concatenate([asm, rng.integers(0, 2, 8272 - 32).astype(np.uint8)]) for _ in range(27)])
    stream = np.concatenate([stream, rng.integers(0, 2, 32 * DATA - len(stream)).astype(np.uint8)])
    words = [enc.encode(stream[k * DATA:(k + 1) * DATA]) for k in range(32)]
    kinds = [0] * 10 + [2] * 6 + [1] * 6 + [3] * 4 + [0] * 6  # CorrelatorGeneric's four OQPSK tables; 2 and 3: the wrong rail is delayed
    iq = []
    for w, k in zip(words, kinds):
        p = pairs_stream(wire_frame(w, True))
        if k == 0:
            p = np.stack([-p[:, 1], p[:, 0]], axis=1)
        elif k == 1:
            p = np.stack([p[:, 1], -p[:, 0]], axis=1)
        elif k == 3:
            p = -p
        iq.append((p, k))
    out = []
    for p, k in iq:
        if k >= 2:  # Q one symbol late inside the stretch (the module shifts it back and loses the frame's last Q)
            p = p.copy()
            p[:, 1] = np.concatenate([[0.0], p[:-1, 1]])
        out.append(p)
    v = np.concatenate(out).reshape(-1) * AMP
    sig = np.full(len(v), SIGMA)
    sig[27 * F:28 * F] = 110.0
    s = quantise(v + sig * rng.standard_normal(len(v)))
    return s, words, dict(kinds=kinds, noisy=[27])


def make_bpsk(enc, rng):
    words = [enc.encode(rng.integers(0, 2, DATA).astype(np.uint8)) for _ in range(16)]
    v = np.concatenate([wire_frame(w, False).astype(np.float64) * 2.0 - 1.0 for w in words])
    v[8 * F:] *= -1.0  # inverted halfway
    s = quantise(v * AMP + 22.0 * rng.standard_normal(len(v)))
    return s, words, dict(inverted_from=8)


# ---- the int8 rails: streams quantised to the whole int8 range, strong enough to saturate. rotate_soft turns every -128 into -127 (rotation.cpp:9-11) before the
# turn; derand_ccsds_soft then complements the bytes under a PN one, so that every 127 of such a byte reaches CCSDSLDPC::decode as -128
AMP_R, SIGMA_R = 90.0, 36.0  # some 7 % of the bytes at each rail, some 50 hard-decision errors in a frame


def quantise_rails(v: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(v), -128, 127).astype(np.int8)


def make_rails_qpsk(enc, rng):
    words = [enc.encode(rng.integers(0, 2, DATA).astype(np.uint8)) for _ in range(12)]
    turns = [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    iq = []
    for w, t in zip(words, turns):
        p = pairs_stream(wire_frame(w, True))
        for _ in range(t):
            p = np.stack([-p[:, 1], p[:, 0]], axis=1)
        iq.append(p)
    v = np.concatenate(iq).reshape(-1) * AMP_R
    return quantise_rails(v + SIGMA_R * rng.standard_normal(len(v))), words, dict(turns=turns, amp=AMP_R, sigma=SIGMA_R)


def make_rails_oqpsk(enc, rng):
    words = [enc.encode(rng.integers(0, 2, DATA).astype(np.uint8)) for _ in range(4)]
    kinds = [2, 2, 3, 3]  # the tables whose Q rail the module shifts back
    out = []
    for w, k in zip(words, kinds):
        p = pairs_stream(wire_frame(w, True))
        if k == 3:
            p = -p
        p = p.copy()
        p[:, 1] = np.concatenate([[0.0], p[:-1, 1]])
        out.append(p)
    v = np.concatenate(out).reshape(-1) * AMP_R
    return quantise_rails(v + SIGMA_R * rng.standard_normal(len(v))), words, dict(kinds=kinds, amp=AMP_R, sigma=SIGMA_R)


def make_rails_bpsk(enc, rng):
    words = [enc.encode(rng.integers(0, 2, DATA).astype(np.uint8)) for _ in range(4)]
    v = np.concatenate([wire_frame(w, False).astype(np.float64) * 2.0 - 1.0 for w in words])
    v[2 * F:] *= -1.0
    return quantise_rails(v * AMP_R + SIGMA_R * rng.standard_normal(len(v))), words, dict(inverted_from=2, amp=AMP_R, sigma=SIGMA_R)


def words_decoded(frames: np.ndarray, words) -> list:
    sent = {packed_frame(w): i for i, w in enumerate(words)}
    return [sent.get(f[4:].tobytes(), -1) for f in frames.reshape(-1, 1024)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ldpc"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    enc = Encoder()
    index = ["# produced by tools/gen_ccsds_ldpc_golden.py from the reference's own sources (ccsds_ldpc_decoder, ldpc_rate 7/8); name, size, key:sha256[:12]"]
    seen_sync = {BPSK: set(), QPSK: set(), OQPSK: set()}

    def save(name, arrays):
        path = os.path.join(args.out, name + ".npz")
        save_npz(path, arrays)
        size = os.path.getsize(path)
        assert size <= 512 * 1024, (name, size)
        index.append(f"{name}.npz {size:9d} B  " + " ".join(f"{k}:{sha(v)}" for k, v in sorted(arrays.items())))
        return size

    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(args.ref, tmp)
        cases = []
        rng = np.random.default_rng(7801)
        s, words, how = make_qpsk_direct(enc, rng)
        cases.append(("r78_qpsk_direct", dict(constellation=QPSK, derandomize=1, iterations=10, internal_stream=0), s, words, how))
        rng = np.random.default_rng(7802)
        s, words, how = make_oqpsk_internal(enc, rng)
        cases.append(("r78_oqpsk_internal", dict(constellation=OQPSK, derandomize=1, iterations=10, internal_stream=1, internal_cadu_size=8272, internal_asm=0x352EF853), s, words, how))
        rng = np.random.default_rng(7803)
        s, words, how = make_bpsk(enc, rng)
        cases.append(("r78_bpsk", dict(constellation=BPSK, derandomize=0, iterations=3, internal_stream=0), s, words, how))
        rng = np.random.default_rng(7804)
        cases.append(("r78_noise", dict(constellation=QPSK, derandomize=1, iterations=10, internal_stream=0), rng.integers(-127, 128, 12 * F).astype(np.int8), [], dict(noise=True)))
        rng = np.random.default_rng(7806)
        s, words, how = make_rails_qpsk(enc, rng)
        cases.append(("r78_rails", dict(constellation=QPSK, derandomize=1, iterations=10, internal_stream=0), s, words, how))
        rng = np.random.default_rng(7807)
        s, words, how = make_rails_oqpsk(enc, rng)
        cases.append(("r78_rails_oqpsk", dict(constellation=OQPSK, derandomize=1, iterations=10, internal_stream=0), s, words, how))
        rng = np.random.default_rng(7808)
        s, words, how = make_rails_bpsk(enc, rng)
        cases.append(("r78_rails_bpsk", dict(constellation=BPSK, derandomize=0, iterations=10, internal_stream=0), s, words, how))
        # r78_rails' unit part: prepared codewords as CCSDSLDPC::decode may receive them, -128 among them
        rng = np.random.default_rng(7809)
        rw = [enc.encode(rng.integers(0, 2, DATA).astype(np.uint8)) for _ in range(8)]
        rcw = np.stack([quantise_rails((np.concatenate([w[LEAD:], [0, 0]]).astype(np.float64) * 2.0 - 1.0) * AMP_R + SIGMA_R * rng.standard_normal(CW)) for w in rw])
        assert (rcw == -128).mean() >= 0.05, (rcw == -128).mean()
        rails_unit = dict(rails_codewords=rcw, rails_words=np.packbits(np.stack([w[LEAD:] for w in rw]), axis=1))
        rright = {}
        for it in (1, 10):
            bits = np.zeros((8, CW), np.uint8)
            corr = np.zeros(8, np.int32)
            L.ldpcref_unit(rcw.ctypes.data, 8, it, bits.ctypes.data, corr.ctypes.data)
            assert bits.max() <= 1
            rails_unit[f"rails_bits_{it}"] = np.packbits(bits, axis=1)
            rails_unit[f"rails_corrections_{it}"] = corr
            rright[it] = np.array([np.array_equal(bits[k, :CW - 2], rw[k][LEAD:]) for k in range(8)])
        assert rright[10].sum() >= 4 and (rright[10] & ~rright[1]).any(), (rright[1], rright[10])
        for name, p, soft, words, how in cases:
            n = len(soft)
            whole = run_module(L, p, soft, extras=True)
            for cuts in ([n // 3, n // 3 + 12345], [1, 7, 8191, 8192, 8193, 40000, 40001, n - 1], list(range(777, n, 5003))):
                assert same(whole, run_module(L, p, soft, cuts=cuts)), f"{name}: the restated loop's output DEPENDS on how the input is cut ({cuts[:3]}...)"
            seen_sync[p["constellation"]] |= set(int(x) for x in whole["sync"])
            arrays = dict(soft=soft, params=np.frombuffer(json.dumps(dict(p, how=how)).encode(), dtype=np.uint8), **whole)
            slid = np.flatnonzero(whole["locked"] == 0)
            if len(slid):  # the stream cut inside the first slide's extra read: the module has the correlator's answer, the frame is not there yet
                k = int(slid[0])
                read_start = int(whole["offset"][k - 1]) + F if k else 0
                tl = read_start + F + (int(whole["offset"][k]) - read_start) // 2
                t = run_module(L, p, soft[:tl])
                assert len(t["offset"]) == k and t["stats"][0] == 0
                arrays.update(trunc_len=np.array([tl], np.int64), trunc_stats=t["stats"], trunc_cor=t["stat_cor"])
            direct = whole if not p["internal_stream"] else run_module(L, p, soft, internal=0)
            if p["internal_stream"]:
                arrays["frames"] = direct["out"]
            line = f"{name}: {len(whole['offset'])} frames, {int((whole['locked'] == 0).sum())} slid, sync {sorted(set(whole['sync'].tolist()))}"
            if words:
                ids = words_decoded(direct["out"], words)
                good = sum(1 for i, c in zip(ids, direct["corrections"]) if i >= 0 and c > 0)
                bad = sum(1 for i in ids if i < 0)
                line += f", {good} corrected to the transmitted word, {bad} not decoded"
                if name in ("r78_qpsk_direct", "r78_oqpsk_internal"):
                    assert good >= 16, (name, good)
                    assert bad >= 1, (name, bad)
                assert [i for i in ids if i >= 0] == sorted(set(i for i in ids if i >= 0))
                if name.startswith("r78_rails"):
                    lo, hi = float((soft == -128).mean()), float((soft == 127).mean())
                    line += f", {lo:.3f} of the bytes at -128 and {hi:.3f} at 127"
                    assert lo >= 0.02 and hi >= 0.02, (name, lo, hi)
                    assert good >= (8 if name == "r78_rails" else 2), (name, good)
            if name == "r78_rails":
                arrays.update(rails_unit)
            if name == "r78_noise":
                assert (whole["locked"] == 0).all() and len(whole["offset"]) >= 5, "the noise stream must slide at every read"
            if p["internal_stream"]:
                ncadu = len(whole["out"]) // (p["internal_cadu_size"] // 8)
                line += f", {ncadu} CADUs, deframer state {int(whole['stats'][2])}"
                assert ncadu >= 16
            size = save(name, arrays)
            print(line + f", {size} B; three cuttings leave the output unchanged")
        # ---- unit: prepared codewords (what CCSDSLDPC::decode receives), three noise levels
        rng = np.random.default_rng(7805)
        sig = [14.0] * 5 + [20.0] * 6 + [24.0] * 5
        uw = [enc.encode(rng.integers(0, 2, DATA).astype(np.uint8)) for _ in range(16)]
        cw = np.stack([quantise((np.concatenate([w[LEAD:], [0, 0]]).astype(np.float64) * 2.0 - 1.0) * AMP + sg * rng.standard_normal(CW)) for w, sg in zip(uw, sig)])
        arrays = dict(codewords=cw, sigma=np.array(sig, np.float32), iterations=np.array([1, 10, 25], np.int32), words=np.packbits(np.stack([w[LEAD:] for w in uw]), axis=1))
        right = {}
        for it in (1, 10, 25):
            bits = np.zeros((16, CW), np.uint8)
            corr = np.zeros(16, np.int32)
            L.ldpcref_unit(cw.ctypes.data, 16, it, bits.ctypes.data, corr.ctypes.data)
            assert bits.max() <= 1 and not bits[:, CW - 2:].any()
            arrays[f"bits_{it}"] = np.packbits(bits, axis=1)
            arrays[f"corrections_{it}"] = corr
            right[it] = np.array([np.array_equal(bits[k, :CW - 2], uw[k][LEAD:]) for k in range(16)])
        assert (right[10] & ~right[1]).any(), "r78_unit: no word is right after 10 iterations and wrong after 1"
        Hm = parity_check_matrix()
        arrays["rows"] = np.stack([np.flatnonzero(Hm[r]) for r in range(M)]).astype(np.uint16)
        # a small irregular code: 40 check nodes of 3 .. 9 edges over 96 variable nodes, every variable node used
        gn, gm = 96, 40
        grow = np.full((gm, 32), 0xFFFF, np.uint16)
        for r in range(gm):
            deg = 3 + (r * 5 + 1) % 7
            cols = np.sort(np.concatenate([[(r * 7) % gn, (r * 7 + 3) % gn], rng.choice(gn, deg, replace=False)]))
            cols = np.unique(cols)[:9]
            grow[r, :len(cols)] = cols
        degs = (grow != 0xFFFF).sum(1)
        assert (degs % 2 == 1).any() and (degs % 2 == 0).any() and degs.max() < 32
        gw = quantise(60.0 * rng.standard_normal((12, gn)))
        arrays.update(g_rows=grow, g_nvn=np.array([gn], np.int32), g_words=gw)
        for it in (1, 6):
            gb = np.zeros((12, gn), np.uint8)
            gc = np.zeros(12, np.int32)
            L.ldpcref_generic(grow.ctypes.data, gm, gn, gw.ctypes.data, 12, it, gb.ctypes.data, gc.ctypes.data)
            arrays[f"g_bits_{it}"] = gb
            arrays[f"g_corrections_{it}"] = gc
        assert not np.array_equal(arrays["g_bits_1"], arrays["g_bits_6"])
        size = save("r78_unit", arrays)
        print(f"r78_unit: right after 1 / 10 / 25 iterations: {int(right[1].sum())} / {int(right[10].sum())} / {int(right[25].sum())} of 16, {size} B")
    for c, want in ((BPSK, {0, 1}), (QPSK, {0, 1, 2, 3}), (OQPSK, {0, 1, 2, 3})):
        assert seen_sync[c] == want, (c, seen_sync[c])
    with open(os.path.join(args.out, "INDEX.txt"), "w") as f:
        f.write("\n".join(index) + "\n")


if __name__ == "__main__":
    main()
