"""bench.py --gpus N launches its own ranks (VERDICT r03 missing #1): the launcher branch rehearsed on CPU with gloo."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env, timeout=300):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    env.update(extra_env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_plain_invocation_launches_two_ranks():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"CMTTS_BENCH_DRYRUN": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout          # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["requested"] == 2


def test_full_reaches_every_rank():
    # the launcher hands its argv to the ranks unchanged: each one parses --full (the flag of the extras, roofline_16bit and cpu_baseline)
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--full"], {"CMTTS_BENCH_DRYRUN": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 2, r.stdout


def test_world_size_mismatch_is_refused():
    # the launcher's world size must BE --gpus: a mislabelled number is worse than none
    r = _run(["--gpus", "4"], {"CMTTS_BENCH_DRYRUN": "1", "WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr


def test_too_few_devices_is_refused():
    # no GPU in the CPU container (and one on the GPU box): asking for more than are visible exits non-zero before any work
    import torch
    have = torch.cuda.device_count()
    r = _run(["--gpus", str(have + 1 if have else 2)], {})
    assert r.returncode != 0
    assert "visible" in r.stderr
