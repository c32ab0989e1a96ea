"""bench.py's plain run and its --dump-outputs: a plain run carries the headline figures and none of
the legs behind --full; --steps sets the number of timed steps; two runs with the same arguments
dump the same arrays, and the dumped bodies are the ones the seal kernel writes for those frames
(recomputed here in-process, the first rows also against the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cz_testlib import or_curve_encode

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 4099   # more than the dump's 2048-frame sample, and odd


def _run(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--ramp-ms", "0", "--frames", str(FRAMES), "--dump-outputs", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    import torch
    import bench
    line = _run(tmp_path / "a")
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    # value and ms_per_step describe the same 3 steps (the line rounds them to 3 and 4 decimals)
    ms = line["ms_per_step"]
    assert ms > 1e-3
    gib = FRAMES * 4096 / 2**30
    assert gib / ((ms + 5.1e-5) / 1e3) - 1e-3 <= line["value"] <= gib / ((ms - 5.1e-5) / 1e3) + 1e-3
    for leg in ("cpu_baseline", "seal_open_verify", "scatter_gather"):
        assert not line.get(leg), leg
    roof = line["roofline"]
    assert roof["hbm_copy_GBps"] is None and roof["pmc_build"] is None and roof["kernel_ms"] > 0
    _run(tmp_path / "b")
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    b = {f: np.load(tmp_path / "b" / f) for f in sorted(os.listdir(tmp_path / "b"))}
    assert sorted(a) == sorted(b) == ["bodies.npy", "frame_index.npy"]
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for f in a:
        assert a[f].dtype in (np.float32, np.float64) and np.array_equal(a[f], b[f]), f
    idx = a["frame_index.npy"].astype(np.int64)
    assert 2048 <= len(idx) <= 2050 and idx[0] == 0 and idx[-1] == FRAMES - 1 and np.all(np.diff(idx) > 0)
    # the same workload sealed here: every dumped row is that frame's body
    wl = bench.Workload("4k", FRAMES, 0, torch.device("cuda:0"))
    wl.step()
    torch.cuda.synchronize()
    want = wl.d_out.view(FRAMES, wl.out_stride).cpu().numpy()[idx, :4096 + 33]
    assert a["bodies.npy"].shape == want.shape and np.array_equal(a["bodies.npy"], want.astype(np.float32))
    for row, i in ((0, 0), (len(idx) - 1, FRAMES - 1)):
        payload = wl.d_in[i * wl.in_stride:i * wl.in_stride + 4096].cpu().numpy().tobytes()
        body = or_curve_encode(payload, 1 if i % 8 == 0 else 0, wl.counter0 + i, 0, bench.PRECOM)
        assert a["bodies.npy"][row].astype(np.uint8).tobytes() == body
