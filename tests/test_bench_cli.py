"""bench.py's launch contract on CPU: `--gpus N` without a launcher starts N ranks
itself (a torch.distributed.run child, before any GPU call), the ranks agree on
the world size, and a launcher/flag mismatch fails instead of silently timing
one GPU.  --dry-run stops after rank bring-up (gloo), so no GPU is touched."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        if not env or k not in env:
            e.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          timeout=240, env=e, cwd=ROOT)


def _last_json(out):
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def test_gpus2_self_launches_two_ranks():
    p = _run(["--gpus", "2", "--dry-run"])
    assert p.returncode == 0, p.stderr[-2000:]
    j = _last_json(p.stdout)
    assert j["dry_run"] and j["n_gpus"] == 2 and j["ranks"] == [0, 1] and j["world_sizes_seen"] == [2]


def test_gpus1_dry_run_is_single_rank():
    p = _run(["--dry-run"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert _last_json(p.stdout)["n_gpus"] == 1


def test_launcher_mismatch_fails_loudly():
    p = _run(["--gpus", "2", "--dry-run"], env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0 and "WORLD_SIZE=1" in (p.stderr + p.stdout)


def test_config5_forward_replicas_dry_run():
    """BASELINE configs[4] (cfg5): forward-only replicas, one view per rank at distinct
    yaws, no collective on the data path; the ranks come up and agree (no GPU)."""
    p = _run(["--config", "5", "--gpus", "2", "--dry-run"])
    assert p.returncode == 0, p.stderr[-2000:]
    j = _last_json(p.stdout)
    assert j["config"] == 5 and "replicas" in j["mode"] and "no collective" in j["mode"]
    assert j["n_gpus"] == 2 and j["ranks"] == [0, 1] and j["world_sizes_seen"] == [2]
    assert j["yaws"] == [-20.0, 20.0]
    p1 = _run(["--dry-run"])
    assert _last_json(p1.stdout)["config"] == 3


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("lsr_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_float32_full_and_seeded_sample(tmp_path):
    """--dump-outputs' writer: float32 .npy per array, small arrays whole, an array above
    DUMP_MAX_ELEMS as the same seeded sample of its flattened elements in every call."""
    import numpy as np
    import torch
    bench = _bench_module()
    n = bench.DUMP_MAX_ELEMS + 12345
    big = torch.arange(n, dtype=torch.float64).reshape(1, n) * 0.5
    small = torch.arange(24, dtype=torch.int32).reshape(2, 3, 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), dict(big=big, small=small, absent=None))
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in ("big", "small")}
    assert not (tmp_path / "a" / "absent.npy").exists()
    assert a["small"].dtype == np.float32 and a["small"].shape == (2, 3, 4)
    np.testing.assert_array_equal(a["small"], small.numpy().astype(np.float32))
    assert a["big"].dtype == np.float32 and a["big"].shape == (bench.DUMP_MAX_ELEMS,)
    idx = np.sort(np.random.default_rng(0).integers(0, n, size=bench.DUMP_MAX_ELEMS))
    np.testing.assert_array_equal(a["big"], (idx * 0.5).astype(np.float32))
    np.testing.assert_array_equal(a["big"], np.load(tmp_path / "b" / "big.npy"))
    man = json.load(open(tmp_path / "a" / "manifest.json"))["arrays"]
    assert man["big"]["sampled"] and man["big"]["shape"] == [1, n] and not man["small"]["sampled"]
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 1000 * 1000


def test_full_and_dump_outputs_are_options():
    """--full and --dump-outputs DIR parse (and reach the self-launched ranks); --steps 0
    is refused instead of dividing by zero."""
    p = _run(["--full", "--dump-outputs", "unused_dir", "--gpus", "2", "--dry-run"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert _last_json(p.stdout)["n_gpus"] == 2
    assert not os.path.exists(os.path.join(ROOT, "unused_dir"))
    p = _run(["--steps", "0", "--dry-run"])
    assert p.returncode != 0 and "--steps" in p.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(gpu, tmp_path):
    """A plain run (the small cfg1 workload) prints the headline fields only -- nothing that
    needs runs of its own -- and --dump-outputs writes the last timed step's forward outputs
    and every input's gradient as finite float32 arrays."""
    import numpy as np
    out = tmp_path / "dump"
    p = _run(["--config", "1", "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)])
    assert p.returncode == 0, p.stderr[-2000:]
    j = _last_json(p.stdout)
    assert j["steps"] == 3 and j["warmup"] == 1 and j["unit"] == "frames/s" and j["dtype"] == "f32"
    assert j["higher_is_better"] is True and j["ms_per_step"] > 0
    assert abs(j["value"] * j["ms_per_step"] / 1e3 - 1.0) < 1e-2   # one frame per step on one GPU
    for k in ("stages_ms", "roofline", "hbm_step", "cpu_baseline", "deterministic", "fwd_fps_1mpix", "quick_1mpix"):
        assert k not in j
    names = {f[:-4] for f in os.listdir(out) if f.endswith(".npy")}
    assert names == {"color", "radii", "grad_means3D", "grad_colors_precomp", "grad_opacities", "grad_scales",
                     "grad_rotations", "grad_means2D"}
    for nme in names:
        a = np.load(out / (nme + ".npy"))
        assert a.dtype == np.float32 and np.isfinite(a).all(), nme
    assert np.load(out / "color.npy").shape == (3, 128, 128)
    assert np.abs(np.load(out / "grad_means3D.npy")).max() > 0


@pytest.mark.gpu
def test_full_run_keeps_the_other_figures(gpu):
    """--full (the small cfg1 workload): the headline fields as in a plain run, plus the
    figures measured in runs of their own."""
    p = _run(["--config", "1", "--gpus", "1", "--steps", "3", "--warmup", "1", "--full"])
    assert p.returncode == 0, p.stderr[-2000:]
    j = _last_json(p.stdout)
    assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["unit"] == "frames/s"
    assert set(j["stages_ms"]) >= {"preprocess", "render_fwd", "render_bwd", "preprocess_bwd"}
    assert j["roofline"]["kernel"] in j["stages_ms"] and j["roofline"]["launches_timed"] >= 1
    assert j["hbm_step"]["algorithmic_bytes"] > 0 and j["workload_stats"]["num_rendered"] > 0
    assert j["cpu_baseline"]["value"] > 0 and j["cpu_baseline"]["kind"] == "port"


def test_config1_and_config2_dry_run():
    """BASELINE configs[0] (cfg1: fwd+bwd) and configs[1] (cfg2: forward-only
    replicas) are bench.py lines too."""
    for cfg, mode in ((1, "fwd+bwd"), (2, "replicas")):
        p = _run(["--config", str(cfg), "--dry-run"])
        assert p.returncode == 0, p.stderr[-2000:]
        j = _last_json(p.stdout)
        assert j["config"] == cfg and mode in j["mode"]
