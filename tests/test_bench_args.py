"""CPU: what a plain `bench.py --gpus 1 --steps K --warmup W` starts before it touches the GPU, against a --full run -- main() driven
with the GPU leg and the child processes replaced by recorders (no GPU is touched here)."""
import json
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

DRIVER = textwrap.dedent('''
    import json, sys
    sys.path.insert(0, %r)
    import bench
    started = []

    class Cpu(object):
        def __init__(self, *args):
            started.append("cpu_baseline")

        def abort(self):
            pass

    def achievable_rates():
        started.append("achievable_rates")

    def live_traffic(a, *args, **kw):
        started.append("live_traffic")

    def run(a, rank, world, local, slab_leg, cpu):
        return {"full": a.full, "also": a.also, "started": started, "cpu": cpu is not None}

    bench.CpuBaseline, bench.achievable_rates, bench.live_traffic, bench.run = Cpu, achievable_rates, live_traffic, run
    sys.argv = ["bench.py"] + sys.argv[1:]
    bench.main()
''' % ROOT)


def drive(tmp_path, args):
    p = tmp_path / "drive_bench.py"
    p.write_text(DRIVER)
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "HJ_BENCH_FORCE_SLAB"):
        env.pop(k, None)
    return subprocess.run([sys.executable, str(p)] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_plain_run_starts_no_child_passes(tmp_path):
    r = drive(tmp_path, ["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d == {"full": False, "also": bench.ALSO_DEFAULT, "started": [], "cpu": False}


def test_full_run_starts_the_baseline_and_the_passes(tmp_path):
    r = drive(tmp_path, ["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["full"] is True and d["cpu"] is True
    assert d["started"] == ["cpu_baseline", "achievable_rates", "live_traffic"]


def test_also_without_full_is_refused(tmp_path):
    r = drive(tmp_path, ["--gpus", "1", "--steps", "20", "--warmup", "5", "--also", "C5"])
    assert r.returncode == 2 and "--full" in r.stderr and not r.stdout.strip()
    r = drive(tmp_path, ["--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--also", "C5"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["also"] == "C5"
