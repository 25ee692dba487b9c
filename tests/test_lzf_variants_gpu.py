"""GPU side of the LZF-variant suite: k_lzf_decode on every scripted and re-encoded stream of
tests/lzf_variants.py, through the real path (GenericIndexed blocks, upload_blocks placement, LzfJob, the
consumers), and on the malformed streams it must refuse.

Expected values are the scripts' own plaintext, the spec's arrays and the oracle's reading of the same segment
bytes; test_lzf_variants.py (CPU) holds the streams to the oracle's decoder and counts what they reach."""
import importlib

import numpy as np
import pytest

import lzf_variants as LV
from compare import assert_results

pytestmark = pytest.mark.gpu

FULL = (0, 1 << 40)


@pytest.fixture(scope="module")
def M():
    class Mods:
        R = importlib.import_module("incubator-druid_amd.runners")
        N = importlib.import_module("incubator-druid_amd._native")
        S = importlib.import_module("incubator-druid_amd.segment")
        W = importlib.import_module("incubator-druid_amd.writer")
        Q = importlib.import_module("incubator-druid_amd.query")
    return Mods


def scan(M, seg, columns, flt=None):
    """{column: values} of every (selected) row of one segment, gathered on the device."""
    q = M.Q.ScanQuery(intervals=[FULL], columns=list(columns), filter=flt, limit=0)
    rs = M.R.scan_rows([seg], list(columns), q, q.row_limit, M.R.RunStats())
    try:
        rows = rs.rows(0)
        out = {c: rs.fetch(0, k)[0] for k, c in enumerate(columns)}
    finally:
        rs.close()
    assert all(len(v) == rows for v in out.values())
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


# ----------------------------------------------------------------------------------------------
# scripted long columns: every decoded 8-byte value against the script's plaintext
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("comp", ["lzf", "lzf_v1"])
@pytest.mark.parametrize("group", range(4))
def test_scripted_blocks_bit_exact(M, tmp_path, comp, group):
    names = LV.script_groups(4)[group]
    want = LV.script_values(names)
    hook = LV.script_hook(names)
    spec = M.W.SegmentSpec(timestamps=np.arange(len(want), dtype=np.int64), metrics={"v": ("long", want)})
    p = M.W.write_segment(str(tmp_path / "s"), spec, compression=comp, lzf_encoder=hook)
    assert len(hook.used) == len(names)
    g = M.S.GpuSegment(p)
    try:
        got = scan(M, g, ["v", "__time"])
        assert got["v"].dtype == np.int64 and len(got["v"]) == len(want)
        bad = np.flatnonzero(got["v"] != want)
        if len(bad):  # name the block and the first bytes that differ
            b = int(bad[0]) // 8192
            gb, wb = got["v"][b * 8192:(b + 1) * 8192].tobytes(), want[b * 8192:(b + 1) * 8192].tobytes()
            at = next(i for i in range(LV.BLOCK) if gb[i] != wb[i])
            raise AssertionError(f"{comp} block {names[b]}: {len(bad)} values differ, first at output byte {at}: "
                                 f"got {gb[at:at + 16].hex()} want {wb[at:at + 16].hex()}")
        assert np.array_equal(got["__time"], spec.timestamps)
    finally:
        g.close()


def test_scripted_blocks_per_row_buckets(M, O, tmp_path):
    """Two script blocks through a timeseries with one bucket per row (the route test_gpu_lzf_every_value takes)."""
    names = ["overlaps", "phases00"]
    want = LV.script_values(names)
    spec = M.W.SegmentSpec(timestamps=np.arange(len(want), dtype=np.int64), metrics={"v": ("long", want)})
    p = M.W.write_segment(str(tmp_path / "s"), spec, compression="lzf", lzf_encoder=LV.script_hook(names))
    g = M.S.GpuSegment(p)
    try:
        q = M.Q.TimeseriesQuery(intervals=[(0, len(want))], granularity={"type": "duration", "duration": 1},
                                aggregations=[M.Q.long_sum("v", "v")])
        got = M.R.run_query(q, [g])
        assert np.array_equal(np.array([r.value["v"] for r in got], dtype=np.int64), want)
    finally:
        g.close()


# ----------------------------------------------------------------------------------------------
# re-encoded constrained columns
# ----------------------------------------------------------------------------------------------
def _check_constrained(M, O, path, spec, columns):
    Q = M.Q
    g, o = M.S.GpuSegment(path), O.OracleSegment(path)
    try:
        ts = spec.timestamps
        assert (g.min_time, g.max_time) == (int(ts[0]), int(ts[-1]))
        got = scan(M, g, ["__time"] + columns)
        assert np.array_equal(got["__time"], ts)
        for c in columns:
            if c in spec.dims:
                want = np.asarray(spec.dims[c][1])
                assert np.array_equal(o.ids(c), want)
            else:
                kind, want = spec.metrics[c]
                want = np.asarray(want, dtype={"long": np.int64, "float": np.float32}[kind])
                assert np.array_equal(_bits(o.numeric(c, kind)), _bits(want))
            assert got[c].dtype.itemsize == want.dtype.itemsize and np.array_equal(_bits(got[c]), _bits(want)), c
        sel = scan(M, g, columns, Q.SelectorDimFilter("b", "1"))
        rows = np.flatnonzero(np.asarray(spec.dims["b"][1]) == spec.dims["b"][0].index("1"))
        for c in columns:
            want = np.asarray(spec.dims[c][1] if c in spec.dims else spec.metrics[c][1])[rows]
            assert np.array_equal(_bits(sel[c]), _bits(want.astype(sel[c].dtype))), c
        longs = [c for c in columns if c in spec.metrics and spec.metrics[c][0] == "long"]
        aggs = [Q.count("rows")] + [Q.long_sum(c, c) for c in longs]
        if "f" in columns:
            aggs.append(Q.AggregatorFactory("floatMax", "f", "f"))
        for q in (Q.GroupByQuery(intervals=[FULL], dimensions=["a"], aggregations=aggs),
                  Q.GroupByQuery(intervals=[FULL], dimensions=["b", "a"], aggregations=aggs, granularity="hour"),
                  Q.TimeseriesQuery(intervals=[FULL], granularity="hour", aggregations=aggs)):
            assert_results(q, M.R.run_query(q, [g]), O.run(q, [o]))
        hours = np.unique(ts // 3_600_000)
        assert len(M.R.run_query(Q.TimeseriesQuery(intervals=[FULL], granularity="hour", aggregations=aggs), [g])) == len(hours)
    finally:
        g.close()


@pytest.mark.parametrize("id_bytes", [1, 2, 3, 4])
def test_reencoded_ids_floats_and_time(M, O, tmp_path, id_bytes):
    """Dictionary ids of every width, a float column, a wide long and an LZF __time under every re-encoder; the
    decoded lengths leave remainders 1, 3, 7, 13 and 15 (ids) and 8 (__time) for the byte tail store."""
    for n in LV.CONSTRAINED_ROWS:
        spec = LV.constrained_spec(M.W, n, packed=False)
        for enc in LV.REENCODERS:
            p = M.W.write_segment(str(tmp_path / f"{n}_{enc}"), spec, compression="lzf", id_bytes=id_bytes,
                                  lzf_encoder=LV.REENCODERS[enc])
            _check_constrained(M, O, p, spec, ["a", "b", "wide", "f"])


def test_reencoded_packed_longs(M, O, tmp_path):
    """DELTA (12 bit) and TABLE (4 bit) columns and a DELTA __time: the decoded block is 4 closing bytes longer
    than the bytes the rows need (op > expect_len). (LZF_VERSION columns have no encoding flag: "lzf" only.)"""
    for n in LV.CONSTRAINED_ROWS:
        spec = LV.constrained_spec(M.W, n, packed=True)
        for enc in LV.REENCODERS:
            hook = LV.recording(LV.REENCODERS[enc])
            p = M.W.write_segment(str(tmp_path / f"{n}_{enc}"), spec, compression="lzf", long_encoding="auto", lzf_encoder=hook)
            lens = {len(pl) for pl, _ in hook.seen}
            assert {LV.decoded_lengths(n)["delta12"], LV.decoded_lengths(n)["table4"]} <= lens
            _check_constrained(M, O, p, spec, ["a", "b", "delta", "table"])


def test_value_column_tails(M, O, tmp_path):
    """The byte tail store alone: segments without dictionary ids whose float and 12-bit DELTA blocks end 8, 10, 11
    and 12 bytes past a multiple of 16 (LV.VALUE_TAIL_ROWS), the last values read back by a scan and by sums."""
    Q = M.Q
    for n in LV.VALUE_TAIL_ROWS:
        for packed in (False, True):
            spec = LV.value_tail_spec(M.W, n, packed)
            name = "delta" if packed else "f"
            for enc in ("pieces", "alternating"):
                p = M.W.write_segment(str(tmp_path / f"{n}_{packed}_{enc}"), spec, compression="lzf",
                                      long_encoding="auto" if packed else "longs", lzf_encoder=LV.REENCODERS[enc])
                g, o = M.S.GpuSegment(p), O.OracleSegment(p)
                try:
                    got = scan(M, g, [name, "__time"])
                    want = np.asarray(spec.metrics[name][1])
                    assert np.array_equal(_bits(got[name][-8:]), _bits(want[-8:].astype(got[name].dtype))), (n, name, enc)
                    assert np.array_equal(_bits(got[name]), _bits(want.astype(got[name].dtype))), (n, name, enc)
                    assert np.array_equal(got["__time"], spec.timestamps)
                    agg = Q.long_sum("s", "delta") if packed else Q.AggregatorFactory("floatMax", "s", "f")
                    q = Q.TimeseriesQuery(intervals=[FULL], granularity="all", aggregations=[Q.count("rows"), agg])
                    assert_results(q, M.R.run_query(q, [g]), O.run(q, [o]))
                finally:
                    g.close()


# ----------------------------------------------------------------------------------------------
# malformed streams
# ----------------------------------------------------------------------------------------------
def test_malformed_streams_rejected(M, O, tmp_path):
    """One malformed stream as the only block of a long metric, summed by a timeseries: attach succeeds (an LZF
    block is not walked at attach), the query fails with DG_ERR_FORMAT naming LZF, and a good segment of the
    same context still answers. The kernel refuses each stream before the access the check guards
    (k_lzf_decode in dg_kernels.hip; every read of the stream goes through the staged window, which refill()
    fills from [wb, n) only, zero-padding the last dword and four more):

    * bad magic: `in8(ip) != 'Z' || in8(ip + 1) != 'V'` at the chunk header, after `ip + 5 > n` passed.
    * chunk type 2: `type != 1` once `type == 0` has failed.
    * header cut at 4: `ip + 5 > n`, before any byte of the header is looked at.
    * header cut at 6: `ip + 7 > n`, before the plain length is read.
    * raw chunk past the stream: `ip + len > n`, before the copy from global memory.
    * raw chunk past the block: `op + len > kBlockBytes` in the same comparison, before the copy into LDS.
    * compressed length past the stream: `end > n`.
    * chunk past the block (op + ulen > 65536): `oend > kBlockBytes`.
    * literal run past the chunk: `ip + run > end`, before the run is copied.
    * literal run past the plain length: `op + run > oend`, same comparison.
    * short reference cut, long reference cut at its length / at its offset: `ip > end` after the token's
      2 or 3 bytes are counted; the bytes peeked past the chunk's end lie inside the window or its zero pad.
    * distance op + 1, distance 8192 at op 10: `dist > op`, before outb[op - dist] is formed.
    * reference past the plain length: `op + l > oend`, same comparison.
    * chunk ends before its plain length: `op != oend` after the token loop.
    * 3 trailing bytes: the chunk loop goes round once more and `ip + 5 > n` fails.
    * short (a well-formed stream of 65528 bytes for 8192 rows): `op < j.expect_len` before the store.
    In every case `bad` returns before the stores to dst, so the slot stays unwritten and the consumer, a
    longSum, reads it as data and indexes nothing with it."""
    W, Q = M.W, M.Q
    vals = LV.malformed_values()
    spec = W.SegmentSpec(timestamps=np.arange(len(vals), dtype=np.int64), metrics={"v": ("long", vals)})
    q = Q.TimeseriesQuery(intervals=[FULL], granularity="all", aggregations=[Q.long_sum("v", "v")])
    good = M.S.GpuSegment(W.write_segment(str(tmp_path / "good"), spec, compression="lzf", lzf_encoder=LV.pieces(30000)))
    want = int(vals.sum())
    try:
        assert M.R.run_query(q, [good])[0].value["v"] == want
        for k, (name, stream) in enumerate(LV.malformed().items()):
            hook = LV.script_hook([])
            hook.table[vals.tobytes()] = stream
            p = W.write_segment(str(tmp_path / f"bad{k}"), spec, compression="lzf_v1" if k % 2 else "lzf", lzf_encoder=hook)
            assert len(hook.used) == 1, name
            with pytest.raises(ValueError):
                O.OracleSegment(p).numeric("v", "long")
            g = M.S.GpuSegment(p)  # attach succeeds
            try:
                with pytest.raises(M.N.DruidGpuError, match="corrupt LZF block") as ei:
                    M.R.run_query(q, [g])
                assert ei.value.code == 1 and "DG_ERR_FORMAT" in str(ei.value), name
            finally:
                g.close()
            assert M.R.run_query(q, [good])[0].value["v"] == want, name
    finally:
        good.close()
