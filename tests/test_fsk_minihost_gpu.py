"""fsk_demod_hip / sdpsk_demod_hip through the drop-in boundary on the GPU: tests/minihost (a host built from the reference's own headers) loads the plugin
and runs the module ids file -> file on the inputs of tests/golden/fsk. (The minihost's stand-in list has no entry for the stock ids fsk_demod / sdpsk_demod,
so the `_hip` ids are addressed directly.) The .soft file written is held to the chunk-parallel contract of tests/test_fsk_gpu.py::test_chunk_parallel_mode,
on the soft bytes: the fixture's length, and the share of bytes equal to the fixture's at or above the float symbols' floor less the bytes that sit next to a
quantiser step (a symbol within 1e-5 of the reference's can still fall on the other side of one: at most scale x 1e-5 x the symbols' rms of all bytes)."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import test_fsk_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "minihost", "_build", "minihost")
PLUGIN = os.path.join(ROOT, "plugin", "_build", "libsdhip_support.so")
LIB = os.path.join(ROOT, "satdump_amd", "lib", "libsdhip.so")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    if not (os.path.exists(HOST) and os.path.exists(PLUGIN)):
        pytest.skip("minihost / plugin not prebuilt")
    return HOST


def _run(host, job, tmp_path):
    jp = tmp_path / "job.json"
    jp.write_text(json.dumps(job))
    p = subprocess.run([host, LIB, PLUGIN, "run", str(jp)], capture_output=True, text=True, env=dict(os.environ), timeout=600)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _params(g, fmt):
    c = g["params"]["cfg"]
    p = {"samplerate": int(c["samplerate"]), "symbolrate": int(c["symbolrate"]), "baseband_format": fmt}
    for k in ("rrc_alpha",):
        if k in c:
            p[k] = c[k]
    for k in ("basic_shaping", "dc_block"):
        if k in c:
            p[k] = bool(c[k])
    return p


@pytest.mark.parametrize("case,module,fmt", [("fsk_a", "fsk_demod_hip", "cf32"), ("fsk_a", "fsk_demod_hip", "cs16"), ("sdpsk_c", "sdpsk_demod_hip", "cs16")])
def test_module_file_to_file(host, tmp_path, case, module, fmt):
    g = G._golden(case)
    inp = tmp_path / ("bb." + fmt)
    if fmt == "cs16":
        g["cs16"].tofile(str(inp))
    else:  # the very floats the cs16 reader makes of the fixture's samples
        (g["cs16"].astype(np.float32) * np.float32(1.0 / 32767.0)).tofile(str(inp))
    job = {"mode": "file", "input": str(inp), "output_hint": str(tmp_path / case), "demod": {"module": module, "parameters": _params(g, fmt)}}
    rep = _run(host, job, tmp_path)
    assert rep["demod_class"] == module
    assert rep["soft"].endswith(".soft")
    soft = np.fromfile(rep["soft"], dtype=np.int8)
    assert len(soft) == len(g["soft"])
    scale = 50.0 if g["params"]["kind"] == "fsk" else 400.0
    rms = float(np.sqrt(np.mean(g["syms"].astype(np.float64) ** 2)))
    share = float(np.mean(soft == g["soft"]))
    print(f"{case} {fmt}: share of soft bytes equal to the fixture's = {share:.4f}")
    assert share >= G.FLOOR[case] - scale * 1e-5 * rms
    st = rep["demod_stats"]
    assert np.isfinite(st["peak_snr"]) and st["peak_snr"] > 0 and 0.0 <= st["progress"] <= 1.0
