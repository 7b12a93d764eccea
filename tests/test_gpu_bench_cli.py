"""bench.py's command line on a GPU, at a tiny N and T: a plain run times --steps rounds and prints the
headline line alone (no roofline, extras or CPU baseline: those need --full), and --dump-outputs writes
what the last timed round returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_the_last_round(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    n, steps = 16, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--n-total", str(n), "--T", "10", "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "candidate-images/sec" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    # value = candidates per second of the timed rounds: N / (ms_per_step / 1e3), both rounded in the line
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / n - 1) < 1e-2
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert not {"sweep", "fp32", "legs", "weak_scaling"} & set(line)
    got = {f[:-4]: np.load(tmp_path / "dump" / f) for f in os.listdir(tmp_path / "dump")}
    assert sorted(got) == ["best", "images", "scores"]
    sc, img, best = got["scores"], got["images"], got["best"]
    assert sc.dtype == np.float64 and sc.shape == (n,) and np.isfinite(sc).all()
    assert img.dtype == np.float32 and img.shape == (n, 3, 32, 32) and np.isfinite(img).all()
    assert best.dtype == np.float64 and int(best[0]) == int(np.argmax(sc)) and best[1] == sc.max()
    assert line["config"]["best_candidate"] == [int(best[0]), best[1]]
