"""bench.py's plain run and --dump-outputs. CPU: the dump's sample of a large groupBy result (fixed, seeded,
within the size limit) and the arrays written for a timeseries / topN result. GPU: a plain run at a small
shape prints the headline line alone (nothing of --full in it), runs exactly --steps timed steps, and its
dump holds what the engine returns for the same query over the same segments."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402

# double sums against the engine's own result of a second run: the same positive terms (normal(5000, 1)), at
# most ROWS of them per sum, perhaps added in another order, so both are within ROWS * 2^-53 of the exact sum
ROWS = 2 * 100000
SUM_RTOL = 2 * ROWS * 2.0 ** -53
FULL_ONLY = ("roofline", "phases_ms", "cpu_baseline", "result_checks", "pcie_fetch", "device_probes")


def test_dump_sample_small_result_is_whole():
    assert bench.dump_sample(0, 48) == []
    assert bench.dump_sample(1000, 48) == [(0, 1000)]
    n = bench.DUMP_BYTES // 48
    assert bench.dump_sample(n, 48) == [(0, n)]


def test_dump_sample_large_result_is_fixed_and_bounded():
    n = 99_500_123  # the headline's ~1 group per row, no multiple of the run length
    runs = bench.dump_sample(n, 48)
    assert runs == bench.dump_sample(n, 48)  # the same groups every time
    assert sum(c for _, c in runs) * 48 <= bench.DUMP_BYTES < 64 << 20
    assert sum(c for _, c in runs) * 48 > bench.DUMP_BYTES // 2  # (and no token sample)
    starts = [s for s, _ in runs]
    assert all(a + bench.DUMP_CHUNK <= b for a, b in zip(starts, starts[1:]))  # ascending, disjoint
    assert starts[0] >= 0 and starts[-1] + bench.DUMP_CHUNK <= n
    assert len(runs) > 1 and starts[-1] - starts[0] > n // 2  # spread over the result, not its head


def _load(d):
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert all(a.dtype == np.float64 for a in out.values())
    return out


def test_dump_outputs_rows(tmp_path, Q):
    iv = ["1970-01-01/2020-01-01"]
    ts = Q.TimeseriesQuery(intervals=iv, granularity="hour", aggregations=[Q.count("rows"), Q.double_sum("d")])
    res = [Q.Result(0, {"rows": 3, "d": 1.5}), Q.Result(3_600_000, {"rows": 2, "d": -0.25})]
    bench.dump_outputs(str(tmp_path / "ts"), ts, res, 0, 1)
    got = _load(str(tmp_path / "ts"))
    assert sorted(got) == ["agg_d", "agg_rows", "timestamp"]
    assert got["timestamp"].tolist() == [0.0, 3_600_000.0]
    assert got["agg_rows"].tolist() == [3.0, 2.0] and got["agg_d"].tolist() == [1.5, -0.25]

    tn = Q.TopNQuery(intervals=iv, dimension="dimA", metric="s", threshold=3, aggregations=[Q.long_sum("s")])
    res = [Q.Result(7, [{"dimA": "x", "s": 9}, {"dimA": None, "s": 4}, {"dimA": "y", "s": 4}])]
    bench.dump_outputs(str(tmp_path / "tn"), tn, res, 0, 1)
    got = _load(str(tmp_path / "tn"))
    assert sorted(got) == ["agg_s", "dim_dimA_hash48", "timestamp"]
    assert got["timestamp"].tolist() == [7.0] * 3 and got["agg_s"].tolist() == [9.0, 4.0, 4.0]
    h = got["dim_dimA_hash48"]
    assert h[1] == -1.0 and h[0] != h[2] and all(0 <= v < 2.0 ** 48 for v in (h[0], h[2]))
    assert h[0] == bench._hash48("x")  # a value's number does not depend on the run


def _plain_run(tmp_path, config, steps):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", config, "--rows", "100000",
           "--segments", "2", "--steps", str(steps), "--warmup", "1", "--lz4-mode", "fast", "--data-dir",
           str(tmp_path / "data"), "--dump-outputs", str(out)]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    b = json.loads(lines[0])
    assert [k for k in FULL_ONLY if k in b] == []
    assert b["steps"] == steps and b["warmup"] == 1 and b["n_gpus"] == 1
    assert b["metric"] == "filtered rows aggregated/sec" and b["unit"] == "rows/s" and b["higher_is_better"] is True
    assert b["dtype"] == "int64/f64"
    assert b["ms_per_step"] > 0
    # value = selected rows per second of the timed steps
    assert b["value"] == pytest.approx(b["selected_rows_per_step"] / (b["ms_per_step"] / 1e3), rel=1e-9)
    return b, _load(str(out))


def _segments(tmp_path, config, S):
    rows, nseg, _, cols = bench.CONFIGS[config]
    paths = bench.ensure_segments(str(tmp_path / "data"), 0, 2, 100000, "lz4", "concise", "fast", cols)  # (reused)
    return [S.GpuSegment(p, device=0) for p in paths]


@pytest.mark.gpu
def test_plain_groupby_run_dumps_the_last_steps_groups(tmp_path, Q):
    R = importlib.import_module("incubator-druid_amd.runners")
    S = importlib.import_module("incubator-druid_amd.segment")
    b, got = _plain_run(tmp_path, "groupby", 3)
    assert b["selected_rows_per_step"] == 200000 and b["groups_per_step"] > 100000
    segs = _segments(tmp_path, "groupby", S)
    try:
        query = bench.make_query(Q, "groupby")
        res = R.groupby_run(segs, query)
        part = res.fetch()
        res.release()
    finally:
        for s in segs:
            s.close()
    n = len(part)
    assert got["groups"].tolist() == [float(n)] and n == b["groups_per_step"]
    assert np.array_equal(got["group_index"], np.arange(n, dtype=np.float64))  # (a small result: every group)
    assert np.array_equal(got["time"], np.asarray(part.times, dtype=np.float64))
    for d, dim in enumerate(query.dimensions):
        assert np.array_equal(got[f"dim_{dim}_id"], part.codes[d].astype(np.float64))
    assert np.array_equal(got["agg_sumLongSequential"], np.asarray(part.aggs[0], dtype=np.float64))
    want = np.asarray(part.aggs[1], dtype=np.float64)
    assert np.allclose(got["agg_sumFloatNormal"], want, rtol=SUM_RTOL, atol=0.0)
    assert sorted(got) == sorted(["groups", "group_index", "time", "dim_dimUniform_id", "dim_dimHyperUnique_id",
                                  "agg_sumLongSequential", "agg_sumFloatNormal"])


@pytest.mark.gpu
def test_plain_topn_run_dumps_the_last_steps_rows(tmp_path, Q):
    R = importlib.import_module("incubator-druid_amd.runners")
    S = importlib.import_module("incubator-druid_amd.segment")
    b, got = _plain_run(tmp_path, "topn", 2)
    segs = _segments(tmp_path, "topn", S)
    try:
        query = bench.make_query(Q, "topn")
        rows = R.run_topn(segs, query)[0].value
    finally:
        for s in segs:
            s.close()
    assert len(rows) == 10
    assert got["dim_dimUniform_hash48"].tolist() == [bench._hash48(r["dimUniform"]) for r in rows]
    assert got["agg_sumLongSequential"].tolist() == [float(r["sumLongSequential"]) for r in rows]
    assert np.allclose(got["agg_sumFloatNormal"], [r["sumFloatNormal"] for r in rows], rtol=SUM_RTOL, atol=0.0)
