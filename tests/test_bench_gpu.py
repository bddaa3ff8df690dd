"""bench.py's plain run on the GPU: the headline leg alone, --steps timed steps, and
--dump-outputs writing the arrays the timed path produced in its last step."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    """One plain bench run (256 docs per step, 2 timed steps) with --dump-outputs."""
    out_dir = tmp_path_factory.mktemp("bench") / "outputs"
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--docs", "256", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0]), out_dir, r.stderr


def test_plain_run_times_the_headline_leg_alone(plain_run):
    d, _, stderr = plain_run
    assert d["unit"] == "docs/s" and d["dtype"] == "bf16x3" and d["higher_is_better"] is True
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value is the docs of the timed steps over their time
    assert d["value"] == pytest.approx(256 / (d["ms_per_step"] / 1e3), rel=1e-3)
    # every timed step launched the dominant GEMM once per layer: --steps set the count
    assert d["roofline"]["launches"] == 2 * 12
    assert d["cpu_baseline"] is None
    for side in ("encode_bf16", "encode_fp32", "retrieve", "retrieve_shard", "quantize",
                 "index_create", "index_e2e", "rank_e2e"):
        assert side not in d, side
    assert "bf16x3 encoder ready" in stderr and "bf16 encoder ready" not in stderr


def test_dump_outputs_holds_the_last_steps_impacts(plain_run):
    d, out_dir, _ = plain_run
    assert sorted(p.name for p in out_dir.iterdir()) == ["impacts_bf16x3.npy"]
    a = np.load(out_dir / "impacts_bf16x3.npy")
    assert a.dtype == np.float32 and a.ndim == 1 and a.size > 256
    assert np.isfinite(a).all() and (a > 0).any()
    # the same bytes the result line digests
    assert hashlib.sha1(a.tobytes()).hexdigest() == d["encode_fp32_faithful"]["out_sha1"]
