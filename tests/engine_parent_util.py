"""Shared by tools/gen_engine_parent_golden.py (which records) and tests/test_engine_parent_{gpu,on_twin_cpu}.py (which compare): the cases under which the HOST side
of the demodulator engine -- the schedule "lane per chunk, judge the hand-offs, re-run what failed" of every speculative stage, what each stage carries from one
call to the next, the compaction behind the clock recovery, the DC block's two modes -- is pinned to what the parent of the host-scaffold refactor (966c66d)
computed, byte for byte and launch for launch. Not a test module. A sibling of tests/afc_variants_util.py, whose streams, hashing and twin binding it uses.

Every stream is cut into calls at bounds that are no multiple of 8, so every carried state, filter history and `inc` crosses a ragged boundary. A record holds,
PER CALL (the engine resets its chunk counters at every call): the sha256 of the call's input, of its soft symbols and of its float symbols (or output samples),
the six chunk counters and the number of launches of every kernel (capi.prof_get()'s `launches`: what pins "the same launches" without a clock); beside them the
first HEAD values of the whole stream's outputs, to say where a mismatch begins."""
import json
import os

import numpy as np

from tests import afc_variants_util as A
from tests.afc_variants_util import COUNTERS, HEAD, sha, twin_capi  # noqa: F401  (re-exported)

ROOT = A.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_parent")
FSK_GOLDEN = os.path.join(ROOT, "tests", "golden", "fsk")
CHUNK, WARMUP = A.CHUNK, A.WARMUP
FSK_CHUNK = 4096  # as tests/test_fsk_gpu.py runs the real-valued chain
# qpsk_own_warmup: the level goes x 4 and the carrier steps by STEP_HZ at mid-stream, three samples in front of the last call. Tuned on the parent (host twin;
# the third call's chunks / re-run / forced and launches of k_afc): 12 kHz 105 / 0 / 0, 3 launches; 14 kHz 105 / 1 / 0, 4; 18 kHz 101 / 4 / 0, 8 of which 4 re-runs
# -- the respec hook re-launched the stage three times and the stream learned a longer warm-up (fewer chunks), the clock recovery's hook once --; 20 kHz
# 105 / 6 / 0; 22 kHz 101 / 19 / 1: a boundary let through. 18 kHz it is.
STEP_HZ = 18000.0
STEP_GAIN = 4.0
DC = 0.05 + 0.03j  # qpsk_dc, qpsk_exact_3calls: a constant added to the input


def _psk(stream, calls, cfg=None, **kw):
    base = dict(A.CASES[stream]["cfg"], chunk_len=CHUNK, warmup=WARMUP)
    base.update(cfg or {})
    return dict(kind="psk", stream=stream, calls=calls, cfg=base, **kw)


_HIER = dict(samplerate=6e6, symbolrate=2333333.0, chunk_len=CHUNK)
CASES = {
    "qpsk_3calls": _psk("qpsk", 3),
    "bpsk_3calls": _psk("bpsk_ragged", 3),
    "qpsk_rrc33_3calls": _psk("qpsk", 3, dict(rrc_taps=33)),
    "qpsk_own_warmup": _psk("qpsk", 3, dict(warmup=0), step=True, fixed=True),
    "noise": _psk("qpsk", 2, noise=True, forced=True),
    "bpsk_carrier": dict(kind="psk", stream="carrier", calls=2, cfg=dict(constellation="bpsk", chunk_len=CHUNK)),
    "qpsk_dc": _psk("qpsk", 3, dict(dc_block=1, post_costas_dc=1), dc=True),
    "qpsk_exact_3calls": _psk("qpsk", 3, dict(exact=1, dc_block=1, post_costas_dc=1), dc=True, exact=True),
    "q8": _psk("qpsk", 3, want_syms=False),
    "front": _psk("qpsk", 2, dict(warmup=0), front_only=True),  # (the engine's own warm-ups: with 512 samples the AGC + filter lanes let boundaries through)
    "hier_qpsk": dict(kind="hier", stream="qpsk", calls=3, cfg=dict(_HIER, constellation="qpsk")),
    "hier_bpsk": dict(kind="hier", stream="bpsk_ragged", calls=3, cfg=dict(_HIER, constellation="bpsk")),
    # single blocks: the Gardner clock recovery (mm_p.loop == 1) on the raw samples at twice their level -- its detector's gain goes with the signal POWER: at
    # amplitude 0.25 the stage doubles its warm-up until one chunk is left --, the Costas loop on symbols (sps 1)
    "gardner": dict(kind="block", stream="qpsk", calls=2, block="clock_recovery_gardner_cc", keys=dict(omega=6e6 / 2333333.0), scale=2.0),
    "costas_block": dict(kind="block", stream="symbols", calls=2, block="costas_cc", keys=dict(order=4, loop_bw=0.003)),
}
for _f in ("fsk_a", "fsk_b", "sdpsk_c"):
    CASES[_f + "_1call"] = dict(kind="fsk", stream=_f, calls=1)
    CASES[_f + "_3calls"] = dict(kind="fsk", stream=_f, calls=3)


def bounds(n: int, calls: int) -> list:
    return {1: [0, n], 2: [0, n // 2 + 3, n], 3: [0, n // 3 + 11, n // 2 + 3, n]}[calls]


_fsk_cache = {}


def fsk_golden(name: str) -> dict:
    if name not in _fsk_cache:
        with np.load(os.path.join(FSK_GOLDEN, name + ".npz")) as z:
            g = {k: z[k] for k in z.files}
        g["params"] = json.loads(bytes(g["params"]).decode())
        _fsk_cache[name] = g
    return _fsk_cache[name]


def signal(name: str) -> np.ndarray:
    """The case's input: complex64 samples, or the fsk fixture's interleaved int16."""
    case = CASES[name]
    s = case["stream"]
    if case["kind"] == "fsk":
        return np.array(fsk_golden(s)["cs16"], copy=True)
    if s == "carrier":
        from tests.test_zy_demod_additions_gpu import _carrier_case
        return np.ascontiguousarray(_carrier_case()[0][:160000])
    if s == "symbols":  # QPSK symbols, one sample each, turning at 0.01 rad / sample, a little noise
        n = A.N_RAGGED
        rng = np.random.default_rng(41)
        a = ((rng.integers(0, 2, n) * 2.0 - 1.0) + 1j * (rng.integers(0, 2, n) * 2.0 - 1.0)) / np.sqrt(2.0)
        w = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.05
        return ((a + w) * np.exp(1j * (0.01 * np.arange(n) + 0.3))).astype(np.complex64)
    if case.get("noise"):
        rng = np.random.default_rng(43)
        return (rng.standard_normal(2 * A.N_ALIGNED) * 0.3).astype(np.float32).view(np.complex64)
    x = A.signal(A.CASES[s])
    n = len(x)
    if case.get("step"):
        t = np.arange(n - n // 2, dtype=np.float64)
        x[n // 2:] = (x[n // 2:].astype(np.complex128) * STEP_GAIN * np.exp(2j * np.pi * STEP_HZ / 6e6 * t)).astype(np.complex64)
    if case.get("dc"):
        x = (x + np.complex64(DC)).astype(np.complex64)
    if case.get("scale"):
        x = (x * np.float32(case["scale"])).astype(np.complex64)
    return x


def _counters(st) -> np.ndarray:
    return np.array([getattr(st, k) for k in COUNTERS], dtype=np.int64)


class _Psk:
    def __init__(self, capi, case):
        cfg = case["cfg"]
        if case["stream"] == "carrier":
            from tests.test_zy_demod_additions_gpu import _carrier_case
            cfg = dict(_carrier_case(nframes=1)[1], **cfg)
        self.capi, self.case = capi, case
        self.per_sym = 1 if cfg["constellation"] == "bpsk" else 2
        self.dem = capi.PskDemod(capi.demod_cfg(**cfg), front_only=bool(case.get("front_only")))

    def call(self, torch, d_x, a, b):
        m = b - a
        d_soft = torch.zeros(2 * m + 64, dtype=torch.int8, device="cuda")
        want_syms = self.case.get("want_syms", True)
        d_syms = torch.zeros(2 * (m + 64), dtype=torch.float32, device="cuda")
        ns = self.dem.process_dev(d_x.data_ptr() + 8 * a, m, self.capi.FMT_CF32, d_soft.data_ptr(), 2 * m + 64, d_syms.data_ptr() if want_syms else 0,
                                  m + 64 if want_syms else 0)
        nsym = ns // self.per_sym
        return d_soft[:ns].cpu().numpy(), (d_syms[: 2 * nsym].cpu().numpy() if want_syms else np.zeros(0, np.float32)), self.dem.stats()

    def close(self):
        self.dem.close()


class _Fsk(_Psk):
    def __init__(self, capi, case):
        g = fsk_golden(case["stream"])
        self.capi = capi
        self.dem = capi.FskDemod(capi.fsk_cfg(g["params"]["kind"], **g["params"]["cfg"], chunk_len=FSK_CHUNK))

    def call(self, torch, d_x, a, b):
        m = b - a
        d_soft = torch.zeros(m + 64, dtype=torch.int8, device="cuda")
        d_syms = torch.zeros(m + 64, dtype=torch.float32, device="cuda")
        ns = self.dem.process_dev(d_x.data_ptr() + 4 * a, m, self.capi.FMT_CS16, d_soft.data_ptr(), m + 64, d_syms.data_ptr(), m + 64)
        return d_soft[:ns].cpu().numpy(), d_syms[:ns].cpu().numpy(), self.dem.stats()


class _Ndsp:
    """The hier chain (the handle of tests/test_ndsp_gpu.py's _run_hier) or one member block (satdump_amd.ndsp.SingleBlock): complex samples in, complex out."""

    def __init__(self, capi, case):
        from satdump_amd import ndsp
        if case["kind"] == "hier":
            self.blk = ndsp.PSKDemodHierBlock(capi_mod=capi)
            for k, v in case["cfg"].items():
                if k == "chunk_len":
                    self.blk._cfg.chunk_len = v
                else:
                    assert self.blk.set_cfg(k, v) == ndsp.RES_OK
        else:
            self.blk = ndsp.SingleBlock(case["block"], capi_mod=capi)
            for k, v in case["keys"].items():
                assert self.blk.set_cfg(k, v) == ndsp.RES_OK
            self.blk._cfg.chunk_len = CHUNK

    def call(self, torch, d_x, a, b):
        m = b - a
        d_y = torch.zeros(2 * (m + 64), dtype=torch.float32, device="cuda")
        ns = self.blk.work_dev(d_x.data_ptr() + 8 * a, m, d_y.data_ptr(), m + 64)
        return np.zeros(0, np.int8), d_y[: 2 * ns].cpu().numpy(), self.blk.stats()

    def close(self):
        self.blk.stop()


def run_case(torch, capi, name: str, x: np.ndarray | None = None) -> dict:
    """Run one case on whatever `capi` is bound to (the library on the GPU with torch, the host twin with tests/emu/fake_torch). Returns the record a fixture
    holds; under "_soft" / "_syms" the whole stream's outputs for the caller (not stored)."""
    case = CASES[name]
    x = signal(name) if x is None else x
    raw = np.array(x, copy=True).view(np.int16 if case["kind"] == "fsk" else np.float32)  # (a copy: the tests share their inputs read-only)
    n = len(raw) // 2
    run = {"psk": _Psk, "fsk": _Fsk, "hier": _Ndsp, "block": _Ndsp}[case["kind"]](capi, case)
    d_x = torch.from_numpy(raw).cuda()
    rec, soft_all, syms_all = {}, [], []
    capi.prof_enable(True)
    try:
        for i, (a, b) in enumerate(zip(bounds(n, case["calls"])[:-1], bounds(n, case["calls"])[1:])):
            capi.prof_reset()
            soft, syms, st = run.call(torch, d_x, a, b)
            prof = capi.prof_get()
            names = sorted(prof)
            rec[f"c{i}_input_sha"] = np.array(sha(raw[2 * a: 2 * b]))
            rec[f"c{i}_soft_sha"], rec[f"c{i}_soft_len"] = np.array(sha(soft)), np.array(len(soft))
            rec[f"c{i}_syms_sha"], rec[f"c{i}_syms_len"] = np.array(sha(syms)), np.array(len(syms))
            rec[f"c{i}_counters"] = _counters(st)
            rec[f"c{i}_launch_names"] = np.array(names, dtype="U64")
            rec[f"c{i}_launch_counts"] = np.array([prof[k][1] for k in names], dtype=np.int64)
            soft_all.append(soft)
            syms_all.append(syms)
    finally:
        capi.prof_enable(False)
        run.close()
    soft, syms = np.concatenate(soft_all), np.concatenate(syms_all)
    rec["soft_head"], rec["syms_head"] = soft[:HEAD].copy(), syms[:HEAD].view(np.uint32).copy()
    rec["_soft"], rec["_syms"] = soft, syms
    return rec


def counters(rec: dict) -> list:
    """[{counter: value} per call]"""
    out, i = [], 0
    while f"c{i}_counters" in rec:
        out.append(dict(zip(COUNTERS, (int(v) for v in rec[f"c{i}_counters"]))))
        i += 1
    return out


def launches(rec: dict, i: int) -> dict:
    return dict(zip((str(s) for s in rec[f"c{i}_launch_names"]), (int(v) for v in rec[f"c{i}_launch_counts"])))


def check_conditions(name: str, rec: dict) -> None:
    """What a record must show for its case to exercise what it is there for -- a condition on the INPUTS, checked on the parent when recording and on the stored
    fixture by the tests: no chunk let through unverified (but in `noise`, where some must be), the lanes ran, a re-run where the case is about re-runs."""
    case, cs = CASES[name], counters(rec)
    assert len(cs) == case["calls"]
    if case.get("forced"):
        assert any(c["chunks_forced"] > 0 for c in cs), f"{name}: no chunk was forced {cs}"
    else:
        assert all(c["chunks_forced"] == 0 for c in cs), f"{name}: a chunk was let through unverified {cs}"
    if case.get("fixed"):
        assert any(c["chunks_fixed"] > 0 for c in cs), f"{name}: no chunk was run again {cs}"
    if not case.get("exact"):  # (exact mode: one sequential lane per stage)
        # the shortest call of all (sdpsk_c_3calls' second: 9 831 samples in chunks of 4 096) is three chunks in each of its three lane stages
        assert all(c["chunks"] >= 6 for c in cs), f"{name}: the lanes did not run {cs}"


def load(backend: str, name: str) -> dict:
    with np.load(os.path.join(GOLDEN, f"{backend}_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def compare(rec: dict, want: dict, name: str) -> None:
    """Byte for byte, call by call: inputs, counters, launch counts (where the fixture holds them), the leading values (for a readable first difference), then the
    lengths and hashes of every call's outputs."""
    calls = CASES[name]["calls"]
    for i in range(calls):
        assert str(rec[f"c{i}_input_sha"]) == str(want[f"c{i}_input_sha"]), f"{name} call {i}: the input differs from the one the fixture was recorded on"
    assert counters(rec) == counters(want), f"{name}: counters {counters(rec)} != {counters(want)}"
    for i in range(calls):
        if f"c{i}_launch_names" in want:
            got, exp = launches(rec, i), launches(want, i)
            diff = {k: (got.get(k, 0), exp.get(k, 0)) for k in sorted(set(got) | set(exp)) if got.get(k, 0) != exp.get(k, 0)}
            assert not diff, f"{name} call {i}: launches (now, parent) {diff}"
    for k in ("soft_head", "syms_head"):
        assert len(rec[k]) == len(want[k]), f"{name}: {k} holds {len(rec[k])} values, the fixture {len(want[k])}"
        d = np.flatnonzero(rec[k] != want[k])
        assert len(d) == 0, f"{name}: {k} differs first at value {d[0]} ({len(d)} of {len(want[k])})"
    for k in sorted(want):
        if k.endswith("_sha") or k.endswith("_len"):
            assert str(rec[k]) == str(want[k]), f"{name}: {k} {rec[k]} != {want[k]}"
