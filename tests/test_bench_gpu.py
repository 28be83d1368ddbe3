"""bench.py on the GPU at a small N: a plain run prints the headline line
without the --full legs, and --dump-outputs writes the last timed step's
result row."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_and_dumps_the_last_row(tmp_path):
    n = 8_000_000
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
           "--settle-s", "0", "--rows-per-gpu", str(n), "--dump-outputs", str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 4 and out["unit"] == "rows/s" and out["higher_is_better"] is True and out["dtype"] == "u64"
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - n / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    # the legs beside the headline figure run under --full only
    assert not {"cpu_baseline", "c_host", "rccl_world1"} & set(out)
    s = n * (n - 1) // 2
    want = [s // n, n - 1, 0]
    assert out["result"] == want
    hi, lo = (np.load(out_dir / ("row" + x + ".npy")) for x in ("_hi32", "_lo32"))
    assert [int(h) * 2**32 + int(l) for h, l in zip(hi, lo)] == want
    row = np.load(out_dir / "row.npy")
    assert row.dtype == np.float64 and list(row) == [float(x) for x in want]
