"""CPU side of the LZF-variant suite (tests/lzf_variants.py).

The scripted streams are held to two independent statements of the format: the script's own byte-by-byte
plaintext and the oracle's decoder (O.lzf_decompress, or_lzf_decompress in oracle/druid_oracle.c), so that a
mismatch in test_lzf_variants_gpu.py is the kernel's. A census asserts that the scripts reach the token
lengths, distances, overlap classes, chunk shapes, block ends and window positions that k_lzf_decode treats
differently; it fails when an edit to the scripts lets one go.

compress-lzf itself is not available to these tests. Where the published format description leaves a point
open (a reference that reaches back into the previous chunk's output: both of our decoders measure the
distance from the block's start), the tests pin the agreement of our two decoders, not the library."""
import hashlib
import importlib
import os

import numpy as np
import pytest

import lzf_variants as LV


@pytest.fixture(scope="module")
def walked():
    return {name: LV.walk(s) for name, s in LV.scripts().items()}


def test_builders_known_answers(O):
    """The token and chunk builders against the hand-assembled bytes of tests/test_lzf.py."""
    assert LV.chunk_lzf([LV.lit(b"a"), LV.ref(1, 9)], 10) + LV.chunk_raw(b"xyz") == \
        bytes.fromhex("5a5601000500" "0a" "0061e00000") + bytes.fromhex("5a56000003") + b"xyz"
    run = bytes(range(32))
    assert LV.chunk_lzf([LV.lit(run), LV.ref(16, 3)], 35) == bytes.fromhex("5a560100") + bytes([35, 0, 35, 31]) + run + bytes([0x20, 15])
    assert LV.ref(8192, 264) == bytes([0xFF, 0xFF, 0xFF]) and LV.ref(257, 8) == bytes([0xC1, 0x00])


def test_scripts_decode_to_their_plaintext(O):
    for name, s in LV.scripts().items():
        assert len(s.plain) == LV.BLOCK, name
        assert O.lzf_decompress(bytes(s.stream), LV.BLOCK) == bytes(s.plain), name


def test_scripts_differ_from_the_writer(O):
    T = importlib.import_module("incubator-druid_amd._tools")
    plains = set()
    for name, s in LV.scripts().items():
        assert bytes(s.stream) != T.lzf_compress(bytes(s.plain)), name
        plains.add(bytes(s.plain))
    assert len(plains) == len(LV.scripts())  # the hook tells the blocks apart by their plaintext


def _payloads(W):
    out = {}
    rng = np.random.default_rng(12)
    ids = rng.integers(0, 200, 4111).astype("<u4")
    for nb in (1, 2, 3, 4):
        out[f"id{nb}"] = ids.view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()
    out["delta12"] = W.vsize_pack(rng.integers(0, 4000, 4093).astype(np.uint64), 12)
    out["table4"] = W.vsize_pack(rng.integers(0, 9, 4097).astype(np.uint64), 4)
    out["float"] = rng.normal(3, 1, 16384).astype("<f4").tobytes()
    out["time"] = np.sort(rng.integers(0, 1 << 40, 8192)).astype("<i8").tobytes()
    out["zeros"] = bytes(65536)
    out["one"] = b"x"
    return out


@pytest.mark.parametrize("enc", list(LV.REENCODERS))
def test_reencoders_round_trip(O, W, enc):
    T = importlib.import_module("incubator-druid_amd._tools")
    for name, data in _payloads(W).items():
        stream = LV.REENCODERS[enc](data)
        assert O.lzf_decompress(stream) == data, name
        assert stream != T.lzf_compress(data) or len(data) == 1, name


def test_reencoders_are_what_they_claim(W):
    data = _payloads(W)["float"]

    def chunks(stream):
        out, ip = [], 0
        while ip < len(stream):
            assert stream[ip:ip + 2] == b"ZV"
            out.append(stream[ip + 2])
            ip += 5 + ((stream[ip + 3] << 8) | stream[ip + 4]) + (2 if stream[ip + 2] else 0)
        assert ip == len(stream)
        return out
    assert set(chunks(LV.REENCODERS["all_literal"](data))) == {1}
    assert set(chunks(LV.REENCODERS["raw_only"](data))) == {0} and len(chunks(LV.REENCODERS["raw_only"](data))) > 20
    assert len(chunks(LV.REENCODERS["pieces"](data))) == (len(data) + 99) // 100
    alt = chunks(LV.REENCODERS["alternating"](data))
    assert alt[:4] == [0, 1, 0, 1] and len(alt) == (len(data) + 332) // 333


# ----------------------------------------------------------------------------------------------
# the census
# ----------------------------------------------------------------------------------------------
def _tokens(walked, *kinds):
    return [e for w in walked.values() for e in w if e["kind"] in kinds]


def test_census_lengths_and_distances(walked):
    lits, refs = _tokens(walked, "lit"), _tokens(walked, "ref2", "ref3")
    assert {e["n"] for e in lits} == set(range(1, 33))
    assert {e["n"] for e in refs} == set(range(3, 265))
    assert {e["n"] for e in refs if e["kind"] == "ref2"} == set(range(3, 9))  # short form; the long form's
    assert {e["n"] for e in refs if e["kind"] == "ref3"} == set(range(9, 265))  # extension byte runs 0..255
    assert {e["dist"] for e in refs} >= set(LV.DISTANCES)
    for d in LV.DISTANCES:  # each at a short, a long and the longest reference
        assert {e["n"] for e in refs if e["dist"] == d} >= {3, 8, 9, 264}, d
    assert any(e["dist"] == e["op"] for e in refs)                       # reaches output byte 0
    cross = [e for e in refs if e["op"] - e["dist"] < e["chunk_op"]]     # source starts in an earlier chunk
    assert any(e["op"] == e["chunk_op"] for e in cross)                  # as the chunk's first token
    assert any(e["op"] - e["dist"] + e["n"] > e["chunk_op"] for e in cross)  # and running into its own chunk
    assert any(e["dist"] == 8192 for e in cross)


def test_census_overlaps(walked):
    refs = {(e["dist"], e["n"]) for e in _tokens(walked, "ref2", "ref3")}
    classes = {"dist < length <= 64": lambda d, n: d < n <= 64,
               "dist < length, length > 64": lambda d, n: d < n and n > 64 and d <= 64,
               "64 < dist < length": lambda d, n: 64 < d < n,
               "dist == length": lambda d, n: d == n,
               "length == 2 * dist + 1": lambda d, n: n == 2 * d + 1,
               "dist == 1 at length 264": lambda d, n: (d, n) == (1, 264)}
    assert set(classes) == set(LV.OVERLAPS)
    for name, pred in classes.items():
        assert all(pred(d, n) for d, n in LV.OVERLAPS[name]), name
        assert set(LV.OVERLAPS[name]) <= refs, name
    # the seam between the two copy branches, at both sides of the 64-lane trip
    assert {(64, 64), (65, 65), (63, 64), (65, 66)} <= refs


def test_census_chunks(walked):
    S = LV.scripts()
    sizes = {(c["type"], c["plain"]) for s in S.values() for c in s.chunks}
    assert {(0, 1), (0, 2), (0, 3), (0, 5), (0, 65535), (1, 1), (1, 2), (1, 65535)} <= sizes
    for name, t in (("raw_halves", 0), ("literal_halves", 1)):
        assert [(c["type"], c["plain"]) for c in S[name].chunks] == [(t, 32768), (t, 32768)]
    # two halves of literal runs: 2 x (7 + 32768 + 1024) bytes, more than the block itself
    assert len(S["literal_halves"].stream) == 67_598
    assert len(S["small_chunks"].chunks) > 700
    big = [c for s in S.values() for c in s.chunks if c["only_lit32"]]
    assert max(c["plain"] for c in big) == 63_520 and max(c["comp"] for c in big) == 65_505 <= 0xFFFF
    # raw chunks: one that ends inside the staged window with a type-1 header and token after it, no restage
    # between; one longer than the window, the next header past the old window's end
    inside = past = False
    residues = set()
    for w in walked.values():
        for a, b, c in zip(w, w[1:], w[2:] + [None]):
            if a["kind"] != "hdr5":
                continue
            residues.add(b["ip"] & 3)
            if b["kind"] == "hdr7" and not b["restaged"] and c and not c["restaged"] and b["ip"] < a["we"]:
                inside = True
            if a["n"] > LV.WIN and b["s"] < 0:
                past = True
    assert inside and past and residues == {0, 1, 2, 3}


def test_census_block_ends(walked):
    S = LV.scripts()
    last = {name: w[-1] for name, w in walked.items()}
    assert any(e["kind"] == "lit" and e["n"] == 32 and e["op"] + 32 == LV.BLOCK for e in last.values())
    assert any(e["kind"] == "ref3" and e["n"] == 264 and e["op"] + 264 == LV.BLOCK for e in last.values())
    assert {len(s.stream) % 4 for s in S.values()} == {0, 1, 2, 3}
    for want in ({"lit"}, {"ref3"}):  # the partial last dword of refill, before each kind of last token
        assert {len(S[n].stream) % 4 for n, e in last.items() if e["kind"] in want} == {0, 1, 2, 3}
    # tokens inside the last 48 bytes of their stream, where the window ends with the stream and stays
    tail = [e for n, w in walked.items() for e in w if e["ip"] + LV.MARGIN > len(S[n].stream)]
    assert tail and all(e["at_end"] for e in tail)
    assert any(not e["restaged"] and 0 < e["s"] < LV.MARGIN for e in tail)
    assert {e["kind"] for e in tail} >= {"lit", "ref3", "hdr5", "hdr7"}


def test_census_window_positions(walked):
    """Every token kind and chunk header at the window offsets where the staging rule changes its answer."""
    mid = [e for w in walked.values() for e in w if not e["at_end"] or e["restaged"]]

    def seen(kind, pred=lambda e: True):
        return {e["s"] for e in mid if e["kind"] == kind and pred(e) and 0 < e["s"] <= LV.MARGIN}
    assert seen("lit", lambda e: e["n"] == 32) >= set(LV.TOKEN_S) == set(range(15, 49))
    assert seen("ref3") >= set(LV.FEW_S) and seen("ref2") >= set(LV.FEW_S)
    assert seen("hdr7") >= set(LV.HEADER_S) and seen("hdr5") >= set(LV.HEADER_S)
    # s = 48 is the last start that does not restage; 47 restages
    for kind in ("lit", "ref2", "ref3", "hdr5", "hdr7"):
        assert any(e["s"] == 48 and not e["restaged"] for e in mid if e["kind"] == kind), kind
        assert any(e["s"] == 47 and e["restaged"] for e in mid if e["kind"] == kind), kind
        # every byte phase of the two-dword peek, in a fresh window and deep inside one
        assert {e["phase"] for e in mid if e["kind"] == kind and e["restaged"]} == {0, 1, 2, 3}, kind
        assert {e["phase"] for e in mid if e["kind"] == kind and not e["restaged"]} == {0, 1, 2, 3}, kind
    # no token can start nearer than 15 bytes to a window's end that is not the stream's (see LV.TOKEN_S)
    assert min(e["s"] for e in mid if e["kind"] in ("lit", "ref2", "ref3") and e["s"] > 0) == 15
    # the lead-literal sweep crosses the first window's end (8192) at 32 of the 33 restaging offsets 15..47
    # (token starts are 8 + k + 33 m: one residue per k), found without the model: the first start past 8144
    first = {8192 - min(e["ip"] for e in walked[f"lead{k:02d}"] if e["ip"] > 8192 - LV.MARGIN) for k in range(1, 33)}
    assert len(first) == 32 and first <= set(range(15, 48))
    assert all(walked[f"lead{k:02d}"][1]["n"] == k for k in range(1, 33))


def test_census_decoded_length_remainders():
    """The byte tail store of k_lzf_decode runs for a decoded length that is no multiple of 16."""
    rem = {}
    for n in LV.CONSTRAINED_ROWS:
        assert n < 8192
        for col, length in LV.decoded_lengths(n).items():
            rem.setdefault(length % 16, []).append((col, n))
    assert set(rem) >= {1, 3, 7, 8, 13, 15}, sorted(rem)
    assert {c for c, _ in rem[13] + rem[15] + rem[1]} >= {"id1", "id3"}
    assert any(c in ("delta12", "table4") for r in rem if r % 16 for c, _ in rem[r])


def test_census_value_tails(W):
    tails = set()
    for n in LV.VALUE_TAIL_ROWS:
        assert n % 2 == 0 and (8 * n) % 16 == 0
        ts = LV.value_tail_spec(W, n, True).timestamps
        assert W.choose_long_encoding(ts)[0] == "delta" and W.choose_long_encoding(ts)[1][2] == 24
        assert W.vsize_serialized_size(24, n) % 16 <= 4          # the packed __time's tail: closing bytes only
        fmt, (_, _, bits) = W.choose_long_encoding(LV.value_tail_spec(W, n, True).metrics["delta"][1])
        assert (fmt, bits) == ("delta", 12)
        tails.add(W.vsize_serialized_size(12, n) % 16)
        tails.add(4 * n % 16)
    assert tails == {0, 8, 10, 11, 12}


# ----------------------------------------------------------------------------------------------
# segments
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("comp", ["lzf", "lzf_v1"])
def test_script_segment_round_trip(O, W, tmp_path, comp):
    names = LV.script_groups()[0]
    vals = LV.script_values(names)
    hook = LV.script_hook(names)
    spec = W.SegmentSpec(timestamps=np.arange(len(vals), dtype=np.int64), metrics={"v": ("long", vals)})
    o = O.OracleSegment(W.write_segment(str(tmp_path / "s"), spec, compression=comp, lzf_encoder=hook))
    assert len(hook.used) == len(names)
    assert np.array_equal(o.numeric("v", "long"), vals) and np.array_equal(o.time(), spec.timestamps)


@pytest.mark.parametrize("enc", list(LV.REENCODERS))
def test_constrained_segment_round_trip(O, W, tmp_path, enc):
    n = LV.CONSTRAINED_ROWS[0]
    for packed in (False, True):
        spec = LV.constrained_spec(W, n, packed)
        hook = LV.recording(LV.REENCODERS[enc])
        p = W.write_segment(str(tmp_path / f"s{packed}"), spec, compression="lzf", id_bytes=3,
                            long_encoding="auto" if packed else "longs", lzf_encoder=hook)
        want = LV.decoded_lengths(n)
        lens = sorted(len(pl) for pl, _ in hook.seen)
        if packed:
            assert want["delta12"] in lens and want["table4"] in lens
        else:
            assert lens == sorted([want["id3"], want["id3"], want["float"], want["long"], want["long"]])
        o = O.OracleSegment(p)
        assert np.array_equal(o.time(), spec.timestamps)
        for name, (dictionary, ids) in spec.dims.items():
            assert o.dictionary(name) == dictionary and np.array_equal(o.ids(name), ids), name
        for name, (kind, v) in spec.metrics.items():
            assert np.array_equal(o.numeric(name, kind), v), name


# ----------------------------------------------------------------------------------------------
# the writer hook
# ----------------------------------------------------------------------------------------------
# sha256 of 00000.smoosh of _small_spec written without the hook, taken before the hook existed
DEFAULT_BYTES = {("lzf", "auto"): "8bf8a3de0805b6706602bc7ead27ee0dba42c3eb1a7264a26e8c66285d8d3090",
                 ("lzf_v1", "longs"): "1d3125c64782d96703e1ff575c68a780ab3a62b6b2d2d4ac4c23f84e68520221"}


def _small_spec(W):
    n = 20_001
    r = np.arange(n)
    tags = W.encode_multi_strings([["a", "b"][: i % 3] + ["t%d" % (i % 5)] if i % 11 else [] for i in range(n)])
    return W.SegmentSpec(timestamps=r.astype(np.int64) * 7,
                         dims={"d": W.encode_strings(["v%02d" % (i * i % 23) for i in range(n)]), "tags": tags},
                         metrics={"m": ("long", r * r % 1013), "t": ("long", r % 200),
                                  "w": ("long", ((r.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(2)).astype(np.int64)),
                                  "f": ("float", (r % 97) / 8.0)}, interval=(0, 7 * n))


def _smoosh(path):
    with open(os.path.join(path, "00000.smoosh"), "rb") as f:
        return f.read()


@pytest.mark.parametrize("comp,long_encoding", list(DEFAULT_BYTES))
def test_hook_keeps_the_default_bytes(W, tmp_path, comp, long_encoding):
    T = importlib.import_module("incubator-druid_amd._tools")
    spec = _small_spec(W)
    kw = dict(compression=comp, long_encoding=long_encoding)
    plain = _smoosh(W.write_segment(str(tmp_path / "plain"), spec, **kw))
    assert hashlib.sha256(plain).hexdigest() == DEFAULT_BYTES[(comp, long_encoding)]
    assert _smoosh(W.write_segment(str(tmp_path / "none"), spec, lzf_encoder=None, **kw)) == plain
    # the build's encoder through the hook: the same file, and the hook saw every LZF block of the segment:
    # __time (3), d (1), tags' offsets (2) and values (1), m, t, w (3 each), f (2); under "auto" __time (DELTA, 20 bits) 2,
    # m (DELTA, 12 bits) and t (TABLE) 1 each, w (DELTA, 64 bits: 4096 rows a block) 5
    hook = LV.recording(T.lzf_compress)
    assert _smoosh(W.write_segment(str(tmp_path / "hooked"), spec, lzf_encoder=hook, **kw)) == plain
    assert all(isinstance(pl, bytes) and 0 < len(pl) <= LV.BLOCK for pl, _ in hook.seen)
    assert len(hook.seen) == (15 if long_encoding == "auto" else 18), len(hook.seen)
    other = _smoosh(W.write_segment(str(tmp_path / "other"), spec, lzf_encoder=LV.all_literal, **kw))
    assert other != plain and len(other) > len(plain)
    # the hook is for LZF blocks alone
    lz4 = _smoosh(W.write_segment(str(tmp_path / "lz4"), spec, compression="lz4", lzf_encoder=LV.all_literal))
    assert lz4 == _smoosh(W.write_segment(str(tmp_path / "lz4b"), spec, compression="lz4"))


# ----------------------------------------------------------------------------------------------
# malformed streams
# ----------------------------------------------------------------------------------------------
def test_malformed_streams_are_refused(O, W, tmp_path):
    bad = LV.malformed()
    assert len(bad) == 19
    for name, stream in bad.items():
        if name == "short":  # well formed, but 8 bytes short of the column's block
            assert O.lzf_decompress(stream, LV.BLOCK) == LV.malformed_values().tobytes()[:-8]
            continue
        with pytest.raises(ValueError):
            O.lzf_decompress(stream, LV.BLOCK)
    # and the oracle refuses the column of a segment that holds one
    vals = LV.malformed_values()
    spec = W.SegmentSpec(timestamps=np.arange(len(vals), dtype=np.int64), metrics={"v": ("long", vals)})
    for name in ("short", "3 trailing bytes", "distance op + 1"):
        hook = LV.script_hook([])
        hook.table[vals.tobytes()] = bad[name]
        o = O.OracleSegment(W.write_segment(str(tmp_path / name.replace(" ", "_")), spec, compression="lzf", lzf_encoder=hook))
        assert len(hook.used) == 1
        with pytest.raises(ValueError):
            o.numeric("v", "long")
        assert np.array_equal(o.time(), spec.timestamps)
