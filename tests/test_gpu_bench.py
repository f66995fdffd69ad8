"""bench.py's plain run measures the headline alone: what takes runs of its own (extras, roofline_16bit, cpu_baseline) waits for --full."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_is_headline_only(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID", "CMTTS_FORCE_COLLECTIVE",
              "CMTTS_MULTI_EXTRAS"):
        env.pop(k, None)
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(dump)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["unit"] == "mel-frames/s" and out["dtype"] == "f32" and out["higher_is_better"] is True
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["roofline"]["launches"] > 0          # the headline kernel's events are recorded inside the timed steps
    assert not {"extras", "roofline_16bit", "cpu_baseline"} & set(out)
    assert (dump / "mel.npy").exists() and (dump / "mel_lens.npy").exists()
