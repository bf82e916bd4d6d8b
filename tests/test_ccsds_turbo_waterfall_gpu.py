"""ccsds_turbo_decoder inside the waterfall (run with -m gpu; tests/test_ccsds_turbo_on_twin_cpu.py collects the same functions against the host twin): codewords
that need 3 .. 8 iterations and some that never decode, so the iteration loop, the in-kernel interleaver of the lower code, a-priori values of large magnitude and
batches that do not fill a wave all decide the result. The fixtures (tests/golden/turbo/turbo_iter_*, turbo_combos_*, unlocked_*, r13_b446, r14_b892, r12_b1115) are
recorded by tools/gen_ccsds_turbo_golden.py from the reference's own turbo_decode loop, run by hand over convcode_extrinsic.

What is held where. On the host twin, which links the libm the fixtures were recorded with: the decided bits of EVERY (frame, iteration count) pair, and every
recorded a-priori array bit for bit. On the GPU, whose exp / log are not glibc's: the bits of every STABLE pair -- a pair is stable when two runs of the reference's
loop whose messages were perturbed after every pass by +-2^-43 max(1, |m|) (about four times BCJR_TOLERANCE) both decide the unperturbed bits -- and the recorded
arrays to BCJR_LATE_TOLERANCE. The generator asserts that iterations 1 and 2 of every frame and every iteration from a frame's first clean one onwards are stable;
of the 232 recorded pairs all 232 are (share 1.0), so on the GPU, too, every recorded pair is held. Unstable pairs that differ would be counted and printed, never
used to excuse a stable one."""
import numpy as np
import pytest

from tests import test_ccsds_turbo_gpu as G
from tests.test_ccsds_turbo_gpu import capi, torch_cuda  # noqa: F401  (fixtures)

gpu = pytest.mark.gpu
RATE = {"r12": "1/2", "r13": "1/3", "r14": "1/4", "r16": "1/6"}
K_ITER, K_COMBO = 8, 6
# max |ours - fixture| / max(1, |fixture|) over the sixteen recorded passes of turbo_iter_r12 .. r16 (the iteration before the first clean one and iteration 8,
# upper and lower code, teacher-forced from the recorded input) as measured on an MI355X (profiles/ccsds_turbo_bench.json); the test allows 16 times
# that, the margin test_bcjr_unit gives a different libm, and never more than 1e-9
BCJR_LATE_MEASURED = 1.776e-15
BCJR_LATE_TOLERANCE = min(16 * BCJR_LATE_MEASURED, 1e-9)
ROUNDS_BEFORE_SERIAL = 6  # speculation rounds, one per slide, that CcsdsTurbo::chain spends before k_ct_chain takes over


def _decode_all(torch, capi, rate, base, soft, K):
    """[frame][k - 1][L]: the bits after k = 1 .. K iterations, all frames in one call per k"""
    return np.stack([G._unit_decode(torch, capi, rate, base, k, soft) for k in range(1, K + 1)], axis=1)


def _hold(tag, got, want, stable):
    differ = (got != want).any(-1)
    stable = np.asarray(stable).astype(bool)
    assert differ.shape == stable.shape
    where = [(int(f), int(k) + 1, int((got[f, k] != want[f, k]).sum())) for f, k in zip(*np.nonzero(differ))]
    print(f"{tag}: {int(stable.sum())} of {stable.size} (frame, iteration) pairs are stable; {int((differ & ~stable).sum())} unstable pairs differ; (frame, k, bits) that differ: {where}")
    if G.BACKEND == "twin":
        assert not differ.any(), (tag, where)
    else:
        assert not (differ & stable).any(), (tag, where)


@gpu
@pytest.mark.parametrize("tag", list(RATE))
def test_decode_every_iteration(torch_cuda, capi, tag):  # noqa: F811
    """five base 223 codewords in one call (two workgroups of k_ct_recur, the second with three dead quarter-waves), k = 1 .. 8: at least three of them are first
    clean at an iteration in 3 .. 8, at least one never is"""
    g = G._golden("turbo_iter_" + tag)
    want = np.unpackbits(np.asarray(g["bits"]), axis=2)
    sent = np.unpackbits(np.asarray(g["sent"]), axis=1)
    first = np.asarray(g["first"])
    assert want.shape == (5, K_ITER, 223 * 8) and ((first >= 3) & (first <= K_ITER)).sum() >= 3 and (first == 0).sum() >= 1
    for f in range(5):
        clean = (want[f] == sent[f]).all(1)
        assert (int(np.argmax(clean)) + 1 if clean.any() else 0) == first[f]
    got = _decode_all(torch_cuda, capi, RATE[tag], 223, g["soft"], K_ITER)
    _hold("turbo_iter_" + tag, got, want, g["stable"])


COMBOS = [(t, b) for t in RATE for b in (446, 892, 1115)]


@gpu
@pytest.mark.parametrize("tag,base", COMBOS)
def test_decode_combos(torch_cuda, capi, tag, base):  # noqa: F811
    """every rate with every longer block: one codeword first clean at an iteration in 3 .. 6, k = 1 .. 6"""
    g = G._golden("turbo_combos_b" if tag == "r16" else "turbo_combos_a")
    key = f"{tag}_b{base}_"
    want = np.unpackbits(np.asarray(g[key + "bits"]), axis=1)[None]
    first = int(g[key + "first"][0])
    assert 3 <= first <= K_COMBO and np.array_equal(want[0, first - 1], np.unpackbits(np.asarray(g[key + "sent"]))) and (want[0, first - 2] != want[0, first - 1]).any()
    got = _decode_all(torch_cuda, capi, RATE[tag], base, np.asarray(g[key + "soft"])[None], K_COMBO)
    _hold(key[:-1], got, want, np.asarray(g[key + "stable"])[None])


def _passes(g):
    """(code, stream, input, output) of the recorded passes: the upper and the lower code at the two recorded iterations"""
    p = np.asarray(g["passes"])
    for x in range(2):
        yield 0, g["stream0"], p[x, 0], p[x, 1]
        yield 1, g["stream1"], p[x, 2], p[x, 3]


def _bcjr(torch, capi, rate, code, streams, msgs):
    """sdhip_op_ccsds_turbo_bcjr on a batch: streams [n][..], msgs [n][2][L] -> msgs"""
    n = len(msgs)
    d_s = G._dev(torch, np.asarray(streams, np.float64))
    d_m = G._dev(torch, np.asarray(msgs, np.float64))
    rc = capi.lib().sdhip_op_ccsds_turbo_bcjr(0, capi.CCSDS_TURBO_RATES[rate], 223, code, d_s.data_ptr(), n, d_m.data_ptr())
    assert rc == 0, capi.last_error()
    return d_m.cpu().numpy().reshape(np.shape(msgs))


@gpu
@pytest.mark.parametrize("tag", list(RATE))
def test_bcjr_passes_late_iterations(torch_cuda, capi, tag):  # noqa: F811
    """one convcode_extrinsic pass from the recorded a-priori arrays of a converging frame (teacher-forced): the iteration before its first clean one, and
    iteration 8, where the frame has converged and the arrays hold |m| > 40 (exp_sum adds log(1 + exp(-40)) == 0 there)"""
    g = G._golden("turbo_iter_" + tag)
    assert (np.abs(np.asarray(g["passes"])[1]) > 40.0).any() and int(g["pass_iters"][1]) == K_ITER
    worst = 0.0
    for x, (code, stream, start, want) in enumerate(_passes(g)):
        got = _bcjr(torch_cuda, capi, RATE[tag], code, np.asarray(stream)[None], np.asarray(start)[None])[0]
        want = np.asarray(want)
        assert got.shape == want.shape and np.isfinite(got).all()
        err = G._message_error(got, want)
        worst = max(worst, err)
        print(f"{tag} iteration {int(g['pass_iters'][x // 2])} code {code}: max |m| in {np.abs(start).max():.1f}, out {np.abs(want).max():.1f}; max |ours - fixture| / max(1, |fixture|) = "
              f"{err:.3e}, {int((got.view(np.uint64) != want.view(np.uint64)).sum())} of {got.size} doubles differ")
        if G.BACKEND == "twin":
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (tag, x, err)
        else:
            assert err <= BCJR_LATE_TOLERANCE, (tag, x, err)
    print(f"{tag}: worst {worst:.3e}")


@gpu
@pytest.mark.parametrize("tag", list(RATE))
def test_bcjr_batch_is_per_frame(torch_cuda, capi, tag):  # noqa: F811
    """six frames in one call (a full wave of four and a wave with two dead quarter-waves) and three (one dead quarter-wave): every frame's arrays are, bit for
    bit, those of the same frame passed alone -- on the GPU too: the operations per frame are the same. The frames differ from each other: the eight recorded
    arrays as a-priori values, the constituent stream rotated by one trellis step per frame."""
    g = G._golden("turbo_iter_" + tag)
    p = np.asarray(g["passes"]).reshape(8, 2, -1)
    for code, stream in ((0, np.asarray(g["stream0"])), (1, np.asarray(g["stream1"]))):
        nc = len(stream) // (223 * 8 + 4)
        streams = np.stack([np.roll(stream, nc * f) for f in range(6)])
        msgs = np.stack([p[(3 * f + code) % 8] for f in range(6)])
        alone = np.stack([_bcjr(torch_cuda, capi, RATE[tag], code, streams[f:f + 1], msgs[f:f + 1])[0] for f in range(6)])
        assert len({a.tobytes() for a in alone}) == 6
        for n in (6, 3):
            got = _bcjr(torch_cuda, capi, RATE[tag], code, streams[:n], msgs[:n])
            bad = [f for f in range(n) if not np.array_equal(got[f].view(np.uint64), alone[f].view(np.uint64))]
            assert not bad, (tag, code, n, bad)


@gpu
@pytest.mark.parametrize("name", ["unlocked_r12_b223", "unlocked_r16_b223"])
def test_unlocked_stream(torch_cuda, capi, name):  # noqa: F811
    """ten reads of noise, every one a slide, before three frames: six speculation rounds, then k_ct_chain walks the rest, the frames included"""
    g = G._golden(name)
    pos = np.asarray(g["pos"])
    assert pos[:11].all() and not pos[11:].any() and np.asarray(g["crc_ok"])[10:].all() and len(g["out"]) == 3 * (223 + 4)
    out, descs, st = G._run(torch_cuda, capi, g, [0, len(g["soft"])])
    G._check(g, out, descs, st)
    assert st.chain_serial >= 1 and st.chain_rounds >= ROUNDS_BEFORE_SERIAL, (st.chain_serial, st.chain_rounds)
    G._check(g, *G._run(torch_cuda, capi, g, G._ragged(g)))


@gpu
@pytest.mark.parametrize("name", G.LONG_STREAMS)
def test_stream_needs_its_iterations(torch_cuda, capi, name):  # noqa: F811
    """the module at turbo_iters - 2: the same reads, fewer frames -- the strict subset the reference emits there, byte for byte"""
    g = G._golden(name)
    it = g["params"]["turbo_iters"]
    fb = g["params"]["turbo_base"] + 4
    want, full = np.asarray(g["out_fewer"]), np.asarray(g["out"])
    rows = {r.tobytes() for r in full.reshape(-1, fb)}
    assert it == 5 and 0 < len(want) < len(full) and all(r.tobytes() in rows for r in want.reshape(-1, fb))
    out, descs, st = G._run(torch_cuda, capi, g, [0, len(g["soft"])], iterations=it - 2)
    for name_ in ("offset", "pos", "swapped"):
        assert np.array_equal(descs[name_].astype(np.int64), np.asarray(g[name_]).astype(np.int64)), name_
    assert np.array_equal(descs["cor"].view(np.uint32), np.asarray(g["cor"]).view(np.uint32))
    assert np.array_equal(descs["crc_ok"].astype(np.int64), np.asarray(g["crc_ok_fewer"]).astype(np.int64))
    assert len(out) == len(want) and np.array_equal(out, want)
    assert st.frames_out * fb == len(want) and st.reads == len(g["offset"])
