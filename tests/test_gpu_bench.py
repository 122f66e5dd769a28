"""bench.py on the GPU box: the driver's single-GPU command shape, and
`--gpus 2` on the box's one GPU (the script starts its two ranks itself; they
share the device and exchange over gloo) prints n_gpus 2 with the config-5
pooled workload (BASELINE configs[4], at reduced chain count)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=110):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_two_ranks_one_gpu(gpu):
    j = _bench(["--gpus", "2", "--steps", "8", "--warmup", "2", "--chains", "8192", "--no-extra"])
    assert j["n_gpus"] == 2 and j["steps"] == 8
    assert "configs[4]" in j["config"]["workload"] and "gloo" in j["config"]["parallelism"]
    assert j["pooled"]["chains_total"] == 2 * 8192 and j["pooled"]["sync_every"] == 1
    assert j["value"] > 0 and j["roofline"]["unit"] == "TFLOP/s"


@pytest.mark.timeout(600)
def test_bench_eight_ranks_config5_shape(gpu):
    """`bench.py --gpus 8` at config 5's own shape (8 x 65,536 chains) on the
    box's one GPU, every sub-leg included: the weak pooled headline, K = 16,
    lag-one overlap, the strong-scaling forms over 524,288 chains in total
    and regime A.  The ranks share the device over
    gloo, so the numbers are not a scaling measurement."""
    j = _bench(["--gpus", "8", "--steps", "8", "--warmup", "2", "--full"], timeout=540)
    assert j["n_gpus"] == 8 and "gloo" in j["config"]["parallelism"]
    assert j["pooled"]["chains_total"] == 8 * 65536 and j["pooled"]["chains_per_gpu"] == 65536
    for leg in ("pooled_sync_every_16", "pooled_overlap", "strong_pooled", "strong_pooled_sync_every_16", "regime_a"):
        assert leg in j and j[leg]["value"] > 0, leg
    assert j["strong_pooled"]["chains_total"] == 524288 and j["strong_pooled"]["chains_per_gpu"] == 65536
    assert j["strong_pooled_sync_every_16"]["sync_every"] == 16


def test_bench_one_gpu_headline(gpu):
    j = _bench(["--steps", "5", "--warmup", "2", "--chains", "4096", "--no-extra"])
    assert j["n_gpus"] == 1 and "configs[1]" in j["config"]["workload"]
    assert j["roofline"]["bound"] == "hbm" and 0 < j["roofline"]["frac"] < 1.2


EXTRA_LEGS = ("pooled", "pooled_sync_every_16", "pooled_overlap")


def test_plain_run_is_the_headline_only_and_full_adds_the_legs(gpu):
    """Without --full the line holds the headline (timed over exactly --steps
    steps) and none of the other legs; --full brings them back (ESS and the
    CPU baseline, seconds each, are switched off here to keep the test short)."""
    args = ["--gpus", "1", "--steps", "6", "--warmup", "2", "--chains", "4096"]
    j = _bench(args)
    assert j["steps"] == 6 and j["warmup"] == 2 and j["dtype"] == "f32" and j["higher_is_better"] is True
    assert j["unit"] == "chain-steps/s" and j["value"] > 0
    assert j["value"] == pytest.approx(4096 / (j["ms_per_step"] * 1e-3), rel=1e-9)
    assert j["fused_chain_steps_per_s"] is None and j["ess"] is None and j["cpu_baseline"] is None
    assert not any(leg in j for leg in EXTRA_LEGS)
    f = _bench(args + ["--full", "--no-ess", "--no-cpu-baseline"])
    assert f["fused_chain_steps_per_s"] > 0
    for leg in EXTRA_LEGS:
        assert f[leg]["value"] > 0, leg
    assert {k for k in f if k not in EXTRA_LEGS} == set(j)


def test_dump_outputs_repeatable(gpu, tmp_path):
    """--dump-outputs writes the state the last timed step returned: every
    chain is exactly warmup + steps transitions from the seeded start (the
    clock warm-up's wall-clock number of launches does not enter), so two runs
    with the same arguments write the same bits."""
    import numpy as np
    C, d, steps, warmup = 4096, 64, 5, 2
    runs = []
    for name in ("a", "b"):
        out = tmp_path / name
        j = _bench(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--chains", str(C),
                    "--dump-outputs", str(out)])
        assert j["steps"] == steps and j["clock_warm"]["launches"] > 0
        runs.append({f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))})
    a, b = runs
    shapes = {"i": (C,), "z": (C, d), "potential_energy": (C,), "mean_accept_prob": (C,), "loc": (C, d),
              "scale": (C, d * (d + 1) // 2), "log_step_size": (C,), "as_change": (C,), "rng_key": (C, 2)}
    assert set(a) == set(b) == set(shapes)
    for name, shape in shapes.items():
        assert a[name].shape == shape and a[name].dtype == (np.float64 if name in ("i", "rng_key") else np.float32)
        assert np.isfinite(a[name]).all(), name
        assert a[name].tobytes() == b[name].tobytes(), name
    assert (a["i"] == warmup + steps).all()
    assert 0 < a["mean_accept_prob"].mean() < 1 and np.ptp(a["z"]) > 0
    assert sum(x.nbytes for x in a.values()) <= 64 * 10**6


def test_dump_outputs_samples_large_leaves(gpu, tmp_path):
    """At the headline's own shape the packed factors (545 MB) do not fit the
    64 MB the dump may take: they are written for a fixed sample of chains,
    the other leaves whole."""
    import numpy as np
    j = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    rows = j["dump_outputs"]["rows"]
    assert rows["z"] == rows["loc"] == rows["i"] == 65536 and 1024 <= rows["scale"] < 65536
    total = 0
    for name, n in rows.items():
        x = np.load(tmp_path / (name + ".npy"))
        assert x.shape[0] == n and np.isfinite(x).all()
        total += os.path.getsize(tmp_path / (name + ".npy"))
    assert np.load(tmp_path / "scale.npy").shape == (rows["scale"], 2080)
    assert total <= 64 * 10**6
