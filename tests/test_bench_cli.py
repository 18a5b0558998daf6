"""bench.py's command line: a plain run times the steps and prints the line; --full adds the side measurements and the CPU baselines;
--dump-outputs writes the last timed step's results, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
# a small configs[2]-like workload: 1 Mb, 2,000 seeds
SMALL = ["--genome-len", "1000000", "--repeat-families", "50", "--seeds", "2000", "--max-len", "5000"]


def _bench(args, env=None, timeout=600):
    return subprocess.run([sys.executable, BENCH] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def test_options_listed():
    r = _bench(["--help"], timeout=60)
    assert r.returncode == 0, r.stderr
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup"):
        assert opt in r.stdout


@pytest.mark.parametrize("args", [["--steps", "0"], ["--workload", "c4", "--dump-outputs", "x"], ["--sharded", "--dump-outputs", "x"]])
def test_bad_arguments_refused(args):
    r = _bench(args, timeout=60)
    assert r.returncode == 2, (r.stdout, r.stderr)


def _line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_and_dumped_outputs(tmp_path):
    env = dict(os.environ, LDBG_BENCH_DIR=str(tmp_path / "inputs"))
    dumps = []
    for run in range(2):
        d = tmp_path / ("out%d" % run)
        r = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)] + SMALL, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        out = _line(r.stdout)
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
        assert out["unit"] == "k-mers traversed/s" and out["higher_is_better"] is True and out["dtype"] == "u64"
        assert "cpu_baseline" not in out and out["single_batch"] == {"skipped": "measured with --full"}
        files = {f: np.load(d / f) for f in sorted(os.listdir(d))}
        assert set(files) == {"walk_lengths.npy", "contig_offsets.npy", "kmers_traversed.npy", "contig_sample_walks.npy", "contig_sample.npy"}
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        wl, offs = files["walk_lengths.npy"], files["contig_offsets.npy"]
        assert len(wl) == 2000 and len(offs) == 2001 and offs[0] == 0 and (np.diff(offs) >= 0).all()
        assert files["kmers_traversed.npy"][0] == out["config"]["kmers_traversed_per_step"]
        assert len(files["contig_sample.npy"]) == sum(offs[int(i) + 1] - offs[int(i)] for i in files["contig_sample_walks.npy"]) > 0
        assert set(np.unique(files["contig_sample.npy"]).tolist()) <= set(b"ACGT")
        dumps.append(files)
    for f in dumps[0]:
        np.testing.assert_array_equal(dumps[0][f], dumps[1][f], err_msg=f)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_full_run(tmp_path):
    env = dict(os.environ, LDBG_BENCH_DIR=str(tmp_path / "inputs"))
    r = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--cpu-seconds", "2"] + SMALL, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _line(r.stdout)
    assert out["single_batch"]["ms_per_step"] > 0 and out["host_seeds"]["ms_per_step"] > 0 and out["with_contigs_fetched"]["ms_per_step"] > 0
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline_tuned_all_cores"]["value"] > 0
    n, m = (int(x) for x in out["parity"].split()[0].split("/"))
    assert n == m > 0, out["parity"]
