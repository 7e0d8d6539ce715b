"""bench.py's multi-rank launcher: `bench.py --gpus N` run without an outside
torch.distributed.run must start N ranks itself (as a child process, before any HIP call) so the
driver's 1/2/4/8-GPU line reports N ranks, and a WORLD_SIZE that disagrees with --gpus must fail.
Each rank reports the ROCm runtime it is bound to: never torch's bundled one.
The CPU test stops at --launch-check (no GPU); the GPU test runs a real 2-rank partitioned step
(host transport, both ranks on GPU 0)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert lines, out[-2000:]
    return json.loads(lines[-1])


def _env():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def test_bench_gpus2_launches_two_ranks():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--launch-check"], capture_output=True, text=True,
                       timeout=300, env=_env(), cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == 2
    assert [q["rank"] for q in line["ranks"]] == [0, 1]
    assert [q["local_rank"] for q in line["ranks"]] == [0, 1]
    assert line["parallelism"] == "mesh-partitioned2 (rccl)"
    # each rank: no torch in the process, every runtime object (incl. the dlopened RCCL) from the
    # directory libaa_admm.so was linked against
    for q in line["ranks"]:
        assert q["torch_imported"] is False
        for name, path in q["runtime_bound"].items():
            assert os.path.dirname(path) == line["runtime_expected"], (q["rank"], name, path)
        for name, paths in q["runtime_mapped"].items():
            assert paths and all(os.path.dirname(p) == line["runtime_expected"] for p in paths), (name, paths)


def test_bench_single_gpu_default_is_one_rank():
    r = subprocess.run([sys.executable, BENCH, "--launch-check"], capture_output=True, text=True, timeout=120,
                       env=_env(), cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == 1 and line["parallelism"] == "replicas1"


def test_bench_world_size_mismatch_fails():
    env = dict(_env(), WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--launch-check"], capture_output=True, text=True,
                       timeout=120, env=env, cwd=REPO)
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_bench_gpus2_partitioned_step_on_one_gpu():
    """Two ranks of one partitioned cloth (host transport, same GPU): the line says 2 ranks."""
    r = subprocess.run([sys.executable, "-u", BENCH, "--gpus", "2", "--partition", "host", "--same-device",
                        "--config", "c2", "--nx", "24", "--steps", "1", "--warmup", "1", "--iters", "20",
                        "--no-cpu-baseline", "--eps-steps", "0"],
                       capture_output=True, text=True, timeout=110, env=_env(), cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == 2
    assert line["config"]["parallelism"] == "mesh-partitioned2 (host)"
    assert line["iters_executed"] == 20 and line["value"] > 0


@pytest.mark.gpu
def test_bench_plain_run_times_the_steps_and_dumps_their_outputs(pkg, ctx, tmp_path):
    """A plain run (no --full) times exactly --steps steps, leaves every leg that needs a run of
    its own out of the line, and --dump-outputs writes what the last timed step returned: the
    positions, velocities and residual rows of the same scene stepped through the binding."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, "-u", BENCH, "--gpus", "1", "--config", "c2", "--nx", "24", "--steps", "2",
                        "--warmup", "1", "--iters", "20", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=110, env=_env(), cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _json_line(r.stdout)
    assert line["steps"] == 2 and line["iters_executed"] == 40 and line["value"] > 0
    assert line["ms_per_step"] > 0 and line["unit"] == "ADMM iters/s" and line["dtype"] == "f64"
    for leg in ("roofline", "time_to_eps", "cpu_baseline"):
        assert line[leg] is None, leg
    assert "secondary" not in line
    assert "reference CPU baseline" not in r.stderr
    got = {n[:-4]: np.load(out / n) for n in sorted(os.listdir(out))}
    assert sorted(got) == ["comb", "prim", "v", "x"]
    assert all(a.dtype == np.float64 for a in got.values())
    want, solver = pkg.capi.run_scene(ctx, pkg.scenes.cloth(24, 24, iters=20, n_steps=2))
    solver.close()
    for name in ("x", "v", "prim", "comb"):
        assert got[name].shape == want[-1][name].shape, name
        np.testing.assert_allclose(got[name], want[-1][name], rtol=1e-9, atol=1e-12, err_msg=name)


@pytest.mark.gpu
def test_bench_plain_geometry_run_prints_its_line_and_dumps_the_solution(tmp_path):
    """The geometry configs' plain run: the line without the --full legs, and the last timed
    solve's solution and residual curve under --dump-outputs."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, "-u", BENCH, "--gpus", "1", "--config", "c3", "--nx", "12", "--steps", "2",
                        "--warmup", "1", "--iters", "20", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=110, env=_env(), cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _json_line(r.stdout)
    assert line["steps"] == 2 and line["accepted_iters"] == 40 and line["value"] > 0 and line["ms_per_step"] > 0
    for leg in ("roofline", "run_to_eps", "cpu_baseline"):
        assert line[leg] is None, leg
    x, comb = np.load(out / "x.npy"), np.load(out / "comb.npy")
    assert x.dtype == np.float64 and x.shape == (line["config"]["points"], 3) and np.isfinite(x).all()
    assert comb.dtype == np.float64 and comb.shape == (20,) and np.isfinite(comb).all()


def test_dump_outputs_samples_a_large_array_the_same_way_every_time(tmp_path):
    """--dump-outputs keeps each array within its byte budget by a fixed, sorted row sample."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    rows = b.DUMP_MAX_BYTES // 24 + 1000
    big = np.arange(3 * rows, dtype=np.float32).reshape(rows, 3)
    small = np.arange(5.0)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, a2 = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float64 and a.nbytes <= b.DUMP_MAX_BYTES and a.shape == (b.DUMP_MAX_BYTES // 24, 3)
    assert np.array_equal(a, a2) and np.all(np.diff(a[:, 0]) > 0)        # same rows, in order
    assert np.array_equal(a[:, 1], a[:, 0] + 1)                            # whole rows of the input
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)


def test_time_to_eps_median_counts_unreached_steps():
    """The time-to-epsilon headline is the median over ALL steps with an unreached step ranked
    above every reached one ("> cap"), so a majority of unreached steps yields null instead of the
    median of the survivors."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    m = b.all_steps_median
    assert m([]) is None
    assert m([10.0, 30.0, 20.0]) == 20.0
    assert m([10.0, None, 20.0]) == 20.0            # 10, 20, >cap
    assert m([10.0, None, None]) is None            # the middle step is unreached
    assert m([10.0, 40.0, None, None]) is None      # even count: the upper middle is unreached
    assert m([10.0, 40.0, 30.0, None]) == 35.0
    assert m([None] * 13 + [5.0] * 7) is None       # round 3's 7/20 survivors no longer make a headline
