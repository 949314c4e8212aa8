"""The bench line's contract, checked two ways.

* CPU: the committed evidence (`profiles/r02_bench_<workload>.json` and the rocprof
  summary of the same command) is self-consistent -- the fields the driver and
  the judge read are present, `value`/`roofline` follow from the byte count and
  the timings, and the trace's average k_stream duration agrees with the line's
  `roofline.kernel_ms`.
* GPU: a short `bench.py` run prints one line of the same shape.
"""
import csv
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROF = os.path.join(ROOT, "profiles")
METRIC = "device-resident checksum GB/s over packet batch; % of HBM-read roofline"
TCP1500_BYTES = 1_048_576 * 1500


def check_line(line: dict, steps: int, warmup: int):
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline"):
        assert k in line, k
    assert line["metric"] == METRIC
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True
    assert line["steps"] == steps and line["warmup"] == warmup
    assert line["scaling"] == "weak" and line["vs_baseline"] is None
    assert line["dtype"] == "u16"
    assert "workload" in line["config"] and "model" not in line["config"]
    # every output of the timed batch checked against the reference (round 3 on;
    # round 2's lines checked a side sample in the cpu_baseline leg)
    assert line["verified_bit_exact"] is True
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=2e-3)
    # achieved = algorithmic bytes per launch / the kernel's average launch time;
    # a step (one batch_dev call) is launches_per_step launches of equal size
    nl = r["launches_per_step"]
    assert nl >= 1 and r["kernel_ms_per_launch"] == pytest.approx(r["kernel_ms"] / nl, rel=1e-3)
    assert r["algo_bytes_per_launch"] == line["config"]["bytes_per_gpu"] // nl
    assert r["achieved"] == pytest.approx(
        r["algo_bytes_per_launch"] / (r["kernel_ms_per_launch"] * 1e-3) / 1e9, rel=2e-3)
    # value = whole-job bytes / wall time per step (HIP event timing sits inside it)
    total = line["config"]["bytes_per_gpu"] * line["n_gpus"]
    assert line["value"] == pytest.approx(total / (line["ms_per_step"] * 1e-3) / 1e9,
                                          rel=5e-3)
    assert line["value"] <= r["achieved"] * 1.01
    # SURVEY §8(d)'s figure beside it (round 4 on): summed bytes + 2 B per result
    if "achieved_contract" in r:
        n = line["config"]["descriptors_per_gpu"]
        assert r["contract_bytes_per_launch"] == (line["config"]["bytes_per_gpu"] + 2 * n) // nl
        assert r["achieved_contract"] == pytest.approx(
            r["contract_bytes_per_launch"] / (r["kernel_ms_per_launch"] * 1e-3) / 1e9, rel=2e-3)
        assert r["frac_contract"] == pytest.approx(r["achieved_contract"] / r["peak"], rel=2e-3)
        assert r["achieved"] < r["achieved_contract"] < r["achieved"] * 1.01
        assert (r["traffic"] is None) == (r["traffic_source"] is None)


# workload -> (algorithmic bytes per step, bound on PMC traffic / algorithmic)
ALGO = {"tcp1500": (TCP1500_BYTES, 1.05), "tcp9000": (1_048_576 * 9000, 1.05),
        "mixed": (1_639_948_630, 1.15)}  # mixed: layout + descriptors, DESIGN.md §5
# every committed evidence set (round tag, workload): the bench line, the
# same command's trace and the traced line, and the PMC summary
EVIDENCE = sorted((f[:3], f[len("r0x_bench_"):-len(".json")]) for f in os.listdir(PROF)
                  if f.startswith("r0") and "_bench_" in f and f[len("r0x_bench_"):-len(".json")] in ALGO)
COMMITTED = {f"{tag}_bench_{wl}.json": ALGO[wl] for tag, wl in EVIDENCE if tag >= "r03"}
# the device function AUTO runs for each committed line (bench.py KERNEL_FN)
DOMINANT = {"tcp1500": "k_window", "tcp9000": "k_window", "mixed": "k_flat2"}


def test_profile_scan_reads_every_committed_pmc_file():
    """bench.py takes roofline.traffic from profiles/*pmc*.json: every committed
    file must parse through that scan (other summaries' shapes included), and
    the headline workloads find their PMC traffic."""
    sys.path.insert(0, ROOT)
    import bench

    for wl, fn in (("tcp1500", "k_window"), ("tcp9000", "k_window"), ("mixed", "k_flat2")):
        t = bench.traffic_from_profiles(wl, "auto-u0-w0", fn)
        assert t is not None and t[0] > 0 and os.path.exists(os.path.join(ROOT, t[1])), wl
    assert bench.traffic_from_profiles("hdr20", "auto-u0-w0", "k_lane") is None


@pytest.mark.parametrize("name", sorted(COMMITTED))
def test_committed_bench_line_consistent(name):
    algo, max_ratio = COMMITTED[name]
    with open(os.path.join(PROF, name)) as f:
        line = json.loads(f.read().strip().splitlines()[-1])
    check_line(line, steps=200, warmup=50)
    assert line["n_gpus"] == 1
    assert line["config"]["bytes_per_gpu"] == algo
    per = algo // line["roofline"]["launches_per_step"]
    assert line["roofline"]["algo_bytes_per_launch"] == per
    # the PMC traffic is per launch and within a few % of the algorithmic bytes
    # (committed beside the line; the line itself carries it once that file exists)
    tag, wl = name[:3], name[len("r0x_bench_"):-len(".json")]
    with open(os.path.join(PROF, f"{tag}_pmc_{wl}.json")) as f:
        pmc = json.load(f)["kernels"][0]
    assert pmc["kernel_regex"] == DOMINANT[wl] and pmc["algo_bytes_per_launch"] == per
    assert 1.0 <= pmc["hbm_bytes_per_launch"] / per < max_ratio
    if line["roofline"]["traffic"] is not None:
        assert 1.0 <= line["roofline"]["traffic"] / per < max_ratio
    assert line["diag"]["settle"]["ms"] >= 200  # clock settle before the warm-up
    cb = line["cpu_baseline"]
    assert cb["kind"] in ("reference", "port") and cb["cores"] >= 1
    assert cb["unit"] == "GB/s" and cb["value"] > 0 and cb["sample"]
    # the host's CPU count and model are stated, and the threads
    # used are the CPUs the process may use (affinity mask under the cgroup quota)
    assert cb["nproc"] >= cb["cores_used"] == cb["cores"] and cb["cpu_model"]
    if cb["cgroup_cpu_quota"]:
        assert cb["cores"] <= cb["cgroup_cpu_quota"] + 1
    # the whole timed batch was checked against the reference, on every rank
    assert line["diag"]["verify"]["descriptors"] == line["config"]["descriptors_per_gpu"]
    assert line["diag"]["verify"]["mismatches"] == 0
    assert line["dist"]["world_size"] == 1 and line["roofline"]["frac_aggregate"] > 0


@pytest.mark.parametrize("tag,wl", [e for e in EVIDENCE if e[0] >= "r03"])
def test_committed_trace_matches_bench_line(tag, wl):
    """The rocprofv3 kernel trace of the same command: its average launch
    agrees with the line the traced process printed (same process, 1 %), and
    with the committed un-profiled line within the process-to-process spread
    (the mixed line is bimodal across processes, 6.24 / 6.42
    TB/s, profiler or not; profiles/r03_mixed_spread/)."""
    with open(os.path.join(PROF, f"{tag}_bench_{wl}.json")) as f:
        line = json.loads(f.read().strip().splitlines()[-1])
    with open(os.path.join(PROF, f"{tag}_{wl}_trace_line.json")) as f:
        traced = json.loads(f.read().strip().splitlines()[-1])
    with open(os.path.join(PROF, f"{tag}_{wl}_kernel_stats.csv")) as f:
        rows = {r["Name"]: r for r in csv.DictReader(f)}
    ks = rows[DOMINANT[wl]]
    # the clock-settle steps (~1 000, their count varies with the run) + 50
    # warm-ups + 200 timed steps of the same command, launches_per_step each
    nl = line["roofline"]["launches_per_step"]
    assert traced["roofline"]["launches_per_step"] == nl
    assert traced["config"] == line["config"]
    assert int(ks["Calls"]) >= (250 + 8) * nl
    avg_ms = float(ks["AverageNs"]) * 1e-6
    # the trace's average includes the settle and warm-up launches
    assert avg_ms == pytest.approx(traced["roofline"]["kernel_ms_per_launch"], rel=0.01)
    assert avg_ms == pytest.approx(line["roofline"]["kernel_ms_per_launch"], rel=0.04)


def _bench(args, env_extra=None, timeout=110):
    env = dict(os.environ, **(env_extra or {}))
    env.pop("WORLD_SIZE", None) if "WORLD_SIZE" not in (env_extra or {}) else None
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_bench_self_launch_two_ranks_dry_run():
    """`bench.py --gpus 2` with no torch.distributed launcher starts its two
    ranks itself (gloo rehearsal on the CPU: --dry-run does every step but the
    GPU work) and rank 0 prints one line for the job, naming the world, the
    backend and who launched the ranks."""
    out = _bench(["--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1", "--settle-ms", "0"])
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["dry_run"] is True and line["value"] is None
    assert line["n_gpus"] == 2
    d = line["dist"]
    assert d["world_size"] == 2 and d["backend"] == "gloo" and d["launcher"] == "bench.py"
    assert [r["rank"] for r in d["ranks"]] == [0, 1]
    assert line["cpu_baseline"] is None


@pytest.mark.parametrize("extra", [[], ["--workload", "tcp1500x64m"], ["--origin", "root"]],
                         ids=["weak", "strong64m", "origin_root"])
def test_bench_self_launch_eight_ranks_dry_run(extra):
    """The three 8-rank commands the driver's scaling run can issue (VERDICT
    r04 Next #3): the default weak line, the 64M x 1500 B strong config
    (BASELINE configs[4]) and the root-origin scatter, each `bench.py --gpus
    8` starting its own eight ranks (gloo rehearsal on the CPU, --dry-run):
    one line naming eight ranks, in order, for the whole job."""
    out = _bench(["--gpus", "8", "--dry-run", "--steps", "2", "--warmup", "1", "--settle-ms", "0"] + extra,
                 timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["dry_run"] is True and line["n_gpus"] == 8
    d = line["dist"]
    assert d["world_size"] == 8 and d["backend"] == "gloo" and d["launcher"] == "bench.py"
    assert [r["rank"] for r in d["ranks"]] == list(range(8))
    if "tcp1500x64m" in extra:
        assert line["scaling"] == "strong"


def test_bench_world_mismatch_fails():
    """WORLD_SIZE from a launcher that disagrees with --gpus is an error."""
    out = _bench(["--gpus", "3", "--dry-run", "--steps", "1", "--warmup", "0"],
                 {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert out.returncode != 0
    assert "WORLD_SIZE=2" in out.stderr


def test_bench_rccl_ranks_need_their_own_gpus():
    """Under RCCL (the default backend) N ranks need N visible GPUs: on a box
    with fewer (this container has none) `bench.py --gpus 2` exits non-zero
    instead of timing one GPU twice."""
    import torch

    if torch.cuda.device_count() >= 2:
        pytest.skip("enough GPUs here")
    out = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--settle-ms", "0"])
    assert out.returncode != 0
    assert "GPU" in out.stderr or "HIP device" in out.stderr


@pytest.mark.gpu
def test_bench_self_launch_rccl_refuses_one_gpu():
    """On the one-GPU box: two RCCL ranks cannot each own a GPU, so the run
    fails loudly (no line, non-zero status)."""
    import torch

    if torch.cuda.device_count() >= 2:
        pytest.skip("more than one GPU visible")
    out = _bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--settle-ms", "0"])
    assert out.returncode != 0
    assert "need 2 GPUs" in out.stderr
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_bench_self_launch_gloo_two_ranks_on_one_gpu():
    """`bench.py --gpus 2` launching its own two ranks, rehearsed over gloo on
    the one GPU: one line, n_gpus 2, both ranks' whole timed batches verified
    against the reference, shared_devices reported."""
    out = _bench(["--gpus", "2", "--steps", "5", "--warmup", "2", "--packets", "262144",
                  "--settle-ms", "50", "--full"], {"LVLIP_DIST_BACKEND": "gloo"})
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["dist"]["launcher"] == "bench.py"
    assert line["dist"]["shared_devices"] is True
    assert line["verified_bit_exact"] is True
    assert all(r["verified"] for r in line["dist"]["ranks"])
    assert line["roofline"]["frac_aggregate"] == pytest.approx(line["value"] / 16000.0, rel=1e-3)


@pytest.mark.gpu
def test_bench_short_run_prints_contract_line():
    env = dict(os.environ)
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2",
         "--full", "--no-cpu-baseline"],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    check_line(line, steps=5, warmup=2)
    assert line["config"]["bytes_per_gpu"] == TCP1500_BYTES
    assert line["roofline"]["frac"] > 0.5
    # --full: the verification's record, the read probes and the PMC traffic
    assert line["diag"]["verify"]["descriptors"] == 1_048_576
    assert "read_probe_GBps" in line["diag"] and line["roofline"]["traffic"] > 0


def test_bench_full_is_off_by_default():
    sys.path.insert(0, ROOT)
    import bench

    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run (`--gpus 1 --steps K --warmup W`) times its K steps and
    prints the line: no verification, CPU baseline, read probe or PMC lookup
    (null / absent), the headline fields as ever.  With --dump-outputs it
    writes the last timed step's checksums, which equal the oracle's over the
    same (seeded) batch, so a second run writes the same file."""
    import numpy as np
    import pyoracle
    import workloads

    n = 70_001  # odd, several blocks; 105 MB of packets
    d = tmp_path / "dump"
    out = _bench(["--gpus", "1", "--steps", "4", "--warmup", "1", "--packets", str(n),
                  "--dump-outputs", str(d)])
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["metric"] == METRIC and line["unit"] == "GB/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u16" and line["steps"] == 4 and line["warmup"] == 1
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(n * 1500 / (line["ms_per_step"] * 1e-3) / 1e9, rel=5e-3)
    assert line["verified_bit_exact"] is None and line["cpu_baseline"] is None
    assert "verify" not in line["diag"] and "read_probe_GBps" not in line["diag"]
    assert line["roofline"]["traffic"] is None and line["roofline"]["traffic_source"] is None
    assert line["roofline"]["kernel_ms"] > 0
    assert sorted(os.listdir(d)) == ["checksums.npy"]
    got = np.load(d / "checksums.npy")
    assert got.dtype == np.float32 and got.shape == (n,)
    b = workloads.make("tcp1500", n=n)
    want = pyoracle.batch(b.host_bytes(), b.descs)
    assert np.array_equal(got, want.astype(np.float32))
    assert line["diag"]["dump_outputs"]["values"] == n


def test_bench_dump_samples_a_large_output(tmp_path):
    """Above its share of the 64 MB budget a rank writes a fixed seeded sample
    and the sample's indices (the CPU side of --dump-outputs: no GPU needed)."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench

    n = 1000
    vals = (np.arange(n, dtype=np.uint32) * 65521 % 65536).astype(np.uint16)
    out = torch.from_numpy(vals.view(np.int16).copy())
    small = bench.dump_outputs(str(tmp_path / "a"), out, n, 0, 1)
    assert small["files"] == ["checksums.npy"] and small["values"] == n
    assert np.array_equal(np.load(tmp_path / "a" / "checksums.npy"), vals.astype(np.float32))
    old = bench.DUMP_BYTES
    bench.DUMP_BYTES = 2 * 12 * 100  # two ranks: 100 sampled values each
    try:
        first = None
        for _rep in range(2):  # the same sample every time
            r = bench.dump_outputs(str(tmp_path / "b"), out, n, 1, 2)
            assert r["files"] == ["checksums_rank1.npy", "checksums_rank1_index.npy"] and r["values"] == 100
            idx = np.load(tmp_path / "b" / "checksums_rank1_index.npy")
            got = np.load(tmp_path / "b" / "checksums_rank1.npy")
            assert idx.dtype == np.float64 and got.dtype == np.float32
            assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
            assert np.array_equal(got, vals[idx.astype(np.int64)].astype(np.float32))
            assert first is None or np.array_equal(first, idx)
            first = idx
    finally:
        bench.DUMP_BYTES = old


@pytest.mark.gpu
def test_bench_two_ranks_rehearsal_prints_one_line():
    """The N>1 path (torch.distributed.run, one process per rank, barriers and
    the max-over-ranks time) with 2 ranks sharing the box's one GPU over gloo
    (LVLIP_DIST_BACKEND=gloo): rank 0 prints one line for the whole job."""
    env = dict(os.environ, LVLIP_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
         "--master-addr", "127.0.0.1", "--master-port", "29531",
         os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2",
         "--packets", "262144", "--settle-ms", "50"],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 5 and line["warmup"] == 2
    assert line["config"]["bytes_per_gpu"] == 262144 * 1500
    # whole-job bytes over the slower rank's wall time
    assert line["value"] == pytest.approx(2 * 262144 * 1500 / (line["ms_per_step"] * 1e-3) / 1e9,
                                          rel=5e-3)
    assert line["cpu_baseline"] is None  # rank 0 at N=1 only
