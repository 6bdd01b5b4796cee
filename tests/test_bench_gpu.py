"""bench.py's plain run: the headline line alone, exactly --steps timed steps, and --dump-outputs writing what the last
timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["unit"] == "samples/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["ms_per_step"] > 0
    assert abs(d["value"] - 64 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    for leg in ("event_timing", "roofline", "roofline_stride2_family", "cpu_baseline", "secondary_bf16_ed", "secondary"):
        assert d[leg] is None, leg                     # --full only

    files = {p.name[:-len(".npy")]: np.load(p) for p in out.iterdir()}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert files["fake_notes"].shape == (64, 256, 128)
    for k in ("G.decoder.pre.2.weight", "G.decoder.deconv.1.running_mean", "E_num.net.0.weight", "D.real_fake.weight"):
        assert k in files, sorted(files)
    assert all(np.isfinite(a).all() for a in files.values())
    # the dumped scalars are the ones the line reports (rounded to 5 decimals there)
    for name, key in (("loss_d", "loss_d"), ("g_adv", "g_adv"), ("g_emo", "g_emo")):
        assert abs(float(files[name][0]) - d["losses"][key]) <= 1e-5 + 1e-6 * abs(d["losses"][key]), name
