"""GPU: the two modes of bench.py.  A plain run (`--gpus 1 --steps N --warmup W`) stops at the headline and spends at most 30 s outside its steps;
`--full` adds the checks, the roofline and the other legs after the timed steps."""
import json, os, subprocess, sys, time
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}


def _bench(*flags):
    from conftest import release_gpu_memory; release_gpu_memory()          # the child shares the GPU with what earlier tests left in THIS process
    env = dict(os.environ)
    for v_ in ("WORLD_SIZE", "RANK", "LOCAL_RANK"): env.pop(v_, None)
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(flags), env=env, timeout=900, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0]), wall


def test_plain_run_stops_at_the_headline_within_30_s_outside_its_steps(tmp_path):
    """the default workload (C3, 1 M reads): start to exit of a new process less (steps + warm-up) x ms_per_step is at most 30 s, the line carries the
    headline and what the timed steps recorded, and none of the legs of --full; --dump-outputs still writes the last step's result"""
    steps, warmup = 2, 1
    out, wall = _bench("--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "dump"))
    outside = wall - (steps + warmup) * out["ms_per_step"] / 1e3
    print("plain run: %.1f s in all, %.2f ms per step, %.1f s outside the steps" % (wall, out["ms_per_step"], outside))
    assert outside <= 30.0
    assert HEADLINE <= set(out) and out["unit"] == "reads/s" and out["higher_is_better"] is True and out["value"] > 0
    assert abs(out["value"] - out["config"]["reads_clustered_per_gpu"] / (out["ms_per_step"] / 1e3)) <= 1e-3 * out["value"]
    cfg = out["config"]
    assert set(cfg["stage_s_per_step"]) >= {"cluster", "consensus", "polish"} and "k_poa_tile" in cfg["kernel_ms_per_step"]
    assert out["roofline"] is None and out["cpu_baseline"] is None and cfg["check"] is None and cfg["kernel_ms_per_step_one_lane"] is None
    assert not {"cli", "host_buffers_in", "with_stable_stop"} & set(cfg)
    assert {"rep_of.npy", "center_polished.npy"} <= set(os.listdir(tmp_path / "dump")) and set(cfg["dumped_outputs"]["shapes"]) >= {"rep_of", "center_polished"}


def test_full_run_reports_the_checks_and_every_leg():
    """--full at a tenth of the default size, CPU baseline switched off: the same headline fields, and beside them the checks, the roofline and the legs"""
    out, _ = _bench("--steps", "1", "--warmup", "1", "--reads", "100000", "--full", "--no-cpu-baseline")
    assert HEADLINE <= set(out) and out["cpu_baseline"] is None
    cfg = out["config"]; chk = cfg["check"]
    assert chk["centers"] == 5 and chk["consensus_edit_distance_vs_truth"] == [0, 0, 0, 0, 0] and chk["cluster_purity"] == 1.0
    assert out["roofline"]["kernel"].startswith("k_") and "dp_kernels" in out["roofline"]
    assert cfg["with_stable_stop"]["same_result"] is True and cfg["host_buffers_in"]["same_consensus"] is True
    assert cfg["cli"]["consensus_equals_amplicons"] is True and cfg["cli"]["with_stable_stop"]["consensus_equals_amplicons"] is True

