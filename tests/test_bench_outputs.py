"""bench.py --dump-outputs / --full: the plain run's result line keeps its
fields, --steps sets the timed steps, and the dumped arrays are what the last
timed step left (float32 / float64 .npy, within the 64 MB budget)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_parses_full_and_dump_outputs():
    code = ("import sys, runpy; sys.argv = ['bench.py']; "
            "g = runpy.run_path('bench.py', run_name='not_main'); "
            "a = g['parse'](['--gpus', '1', '--steps', '7', '--warmup', '2']); "
            "assert a.steps == 7 and not a.full and a.dump_outputs is None; "
            "a = g['parse'](['--full', '--dump-outputs', 'd']); "
            "assert a.full and a.dump_outputs == 'd'; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


@pytest.mark.gpu
def test_bench_dump_outputs_tiny(tmp_path):
    B, T, D, n = 256, 26, 128, 128
    out = tmp_path / "dump"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "4",
           "--rows", "tiny", "--batch", str(B), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["steps"] == 3 and res["warmup"] == 4 and res["dtype"] == "bf16"
    assert res["unit"] == "examples/s" and res["higher_is_better"] is True
    assert res["ms_per_step"] > 0
    # value and ms_per_step describe the same timed window
    assert res["value"] == pytest.approx(B / (res["ms_per_step"] / 1e3), rel=0.05)
    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(arrays) == {"logits", "dense_params", "train_loss", "emb_rows_sampled",
                           "emb_rows_updated"}
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), name
        assert np.isfinite(a).all(), name
    assert arrays["logits"].shape == (B,)
    assert arrays["emb_rows_sampled"].shape == (T, n, D)
    assert arrays["emb_rows_updated"].shape == (T, n, D)
    assert arrays["train_loss"].shape == (1,) and 0 < arrays["train_loss"][0] < 5
    # the step ran: the logits are not the zero-initialised buffer
    assert np.abs(arrays["logits"]).max() > 0
    assert np.abs(arrays["dense_params"]).max() > 0
