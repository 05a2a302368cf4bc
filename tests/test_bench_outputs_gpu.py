"""bench.py --dump-outputs: the arrays of the last timed step depend on the arguments alone (not on
how many warmup steps ran) and equal the same steps taken eagerly from the seeded initial state; a plain
run does no validation pass, --full does.  The two benchmark runs are child processes (started together),
so the suite's own process opens no further streams for them."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("loss", "params", "adam_m", "adam_v")
B, STEPS, DRAWS = 8192, 3, 1 << 17


@pytest.mark.gpu
def test_dump_outputs_are_the_last_timed_step(tmp_path):
    import torch

    from euromillioner_amd.models.mlp import FusedSmallMLP

    argv = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--batch", str(B),
            "--draws-per-gpu", str(DRAWS)]
    runs = {"plain": ["--warmup", "1", "--warmup-ms", "0"], "full": ["--warmup", "4", "--warmup-ms", "20", "--full"]}
    procs = {k: subprocess.Popen(argv + extra + ["--dump-outputs", str(tmp_path / k)], cwd=ROOT, text=True,
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE) for k, extra in runs.items()}
    res, got = {}, {}
    for k, p in procs.items():
        out, err = p.communicate(timeout=120)
        assert p.returncode == 0, err[-2000:]
        d = res[k] = json.loads([x for x in out.splitlines() if x.startswith("{")][-1])
        assert d["steps"] == STEPS and d["ms_per_step"] > 0
        assert abs(d["value"] - B / (d["ms_per_step"] / 1000.0)) <= 1e-6 * d["value"]
        got[k] = {n: np.load(tmp_path / k / (n + ".npy")) for n in NAMES}
    assert res["plain"]["val"] == {} and res["plain"]["val_iid"] == {}
    assert res["full"]["val"]["count"] > 0 and res["full"]["val_iid"]["count"] > 0
    assert got["plain"]["loss"].shape == (1,) and got["plain"]["params"].shape == got["plain"]["adam_m"].shape
    for n in NAMES:
        assert got["plain"][n].dtype == np.float32 and np.isfinite(got["plain"][n]).all()
        np.testing.assert_array_equal(got["plain"][n], got["full"][n])

    # the same STEPS steps taken eagerly from the seeded initial state
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    sh = bench._Shards(DRAWS, 0, 1)
    draws, skip = sh.materialize(sh.train, 0, 0.9, torch.device("cuda", 0))
    m = FusedSmallMLP("cuda:0", loss="softmax", lr=3e-3, seed=0)
    for c in range(STEPS):
        loss = m.step(draws, B, offset=skip + c * B)
    torch.cuda.synchronize()
    for n, t in zip(NAMES, (loss, m.params, m.m, m.v)):
        np.testing.assert_array_equal(got["plain"][n], t.reshape(-1).cpu().numpy())
    assert np.abs(got["plain"]["adam_m"]).max() > 0
