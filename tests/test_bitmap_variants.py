"""CPU side of the bitmap-variant suite (tests/bitmap_variants.py).

The variant encoders are held to an independent decoder, the oracle's (O.concise_rows / O.roaring_rows
and OracleSegment.bitmap_rows on the written segment), so that a mismatch in test_bitmap_variants_gpu.py
is the kernel's. A census asserts that the variants and shapes reach every path of the bitmap kernels;
it fails when a change to the shapes or the encoders lets one go.
"""
import hashlib
import os

import numpy as np
import pytest

import bitmap_variants as BV

# The engine's thresholds, restated (incubator-druid_amd/csrc/dg_internal.h: kConcisePieceWords = 4096,
# a Concise bitmap above twice that many words is cut into pieces; kRoaringSplitBytes = 32768, a Roaring
# bitmap above it is cut into its containers. dg_engine.cpp's search plan sends a Concise bitmap of at
# most 64 words to one wave, longer ones to a workgroup; dg_search.hip: kSearchShortRows = 2048, a
# one-fill or run above it is popcounted by the whole wave / workgroup).
CONCISE_WAVE_WORDS = 64
CONCISE_SPLIT_WORDS = 2 * 4096
ROARING_SPLIT_BYTES = 32768
SEARCH_SHORT_ROWS = 2048

CASES = [(name, side) for name in BV.shapes() for side in BV.SIDES]


@pytest.fixture(scope="module")
def encoded():
    """(kind, variant, shape, side) -> bytes, straight from the encoders."""
    out = {}
    for kind, variant in BV.VARIANTS:
        for name, side in CASES:
            out[(kind, variant, name, side)] = BV.ENCODERS[kind][variant](BV.side_rows(BV.shapes()[name], side), BV.N_ROWS)
    return out


@pytest.fixture(scope="module")
def variant_dirs(tmp_path_factory, W):
    base = tmp_path_factory.mktemp("bitmap_variants")
    return {(k, v): BV.write_variant_segment(W, str(base / f"{k}_{v}"), k, v) for k, v in BV.VARIANTS}


def test_shapes_are_what_they_claim():
    s, n = BV.shapes(), BV.N_ROWS
    assert n == 327_717 and n % 31 and n % 32 and n % 65536
    assert 0.49 < s["half"].mean() < 0.51 and 200 < s["sparse"].sum() < 460
    per = lambda m: np.bincount(np.flatnonzero(m) >> 16, minlength=6).tolist()
    assert per(s["cards"]) == [4096, 0, 4097, 0, 65536, 36] and per(~s["cards"])[4:] == [0, 1]
    assert per(s["three"])[3:] == [0, 0, 0] and min(per(s["three"])[:3]) > 0
    assert per(s["four"])[4:] == [0, 0] and min(per(s["four"])[:4]) > 0
    # the runs of "runs" start 1, 30 and 31 bits into a 32-row word and cross a container boundary
    holes = np.flatnonzero(~s["runs"])
    assert {int(h + 1) % 32 for h in holes} >= {1, 30, 31}
    assert any(a >> 16 != (b - 1) >> 16 for a, b in zip(holes[:-1] + 1, holes[1:]))
    assert all(m.any() and not m.all() for m in s.values())


@pytest.mark.parametrize("kind,variant", BV.VARIANTS)
def test_encoders_decode_to_the_shape(O, encoded, kind, variant):
    decode = O.concise_rows if kind == "concise" else O.roaring_rows
    for name, side in CASES:
        want = BV.side_rows(BV.shapes()[name], side)
        got = decode(encoded[(kind, variant, name, side)])
        assert np.array_equal(got, want), (kind, variant, name, side)


@pytest.mark.parametrize("kind,variant", BV.VARIANTS)
def test_segments_decode_to_the_shape(O, variant_dirs, kind, variant):
    seg = O.OracleSegment(variant_dirs[(kind, variant)])
    assert seg.num_rows == BV.N_ROWS
    for name, mask in BV.shapes().items():
        assert seg.dictionary(name) == list(BV.SIDES)
        assert np.array_equal(seg.ids(name) == 0, mask), name
        for idx, side in enumerate(BV.SIDES):
            assert np.array_equal(seg.bitmap_rows(name, idx), BV.side_rows(mask, side)), (kind, variant, name, side)


def test_variants_differ_from_the_canonical_bytes(encoded):
    """Each variant is another encoding somewhere, not the canonical bytes under another name."""
    for kind, variant in BV.VARIANTS:
        if variant != "canonical":
            assert any(encoded[(kind, variant, n, s)] != encoded[(kind, "canonical", n, s)] for n, s in CASES), variant


def test_variant_word_forms(encoded):
    """The Concise variants hold the words they are named for."""
    def words(variant):
        return np.concatenate([BV.concise_words(encoded[("concise", variant, n, s)]) for n, s in CASES])
    canon, lit, c0 = words("canonical"), words("all_literal"), words("count0_fills")
    assert (lit >> 31).all() and (lit == 0x80000000).any() and (lit == 0xFFFFFFFF).any()
    fills = c0[(c0 >> 31) == 0]
    assert ((fills & 0x01FFFFFF) == 0).all()
    for w in (0x00000000, 0x40000000):
        assert (fills == w).any()
    pos = (fills >> 25) & 0x1F
    assert ((fills >> 30 == 0) & (pos > 0)).any() and ((fills >> 30 == 1) & (pos > 0)).any()
    # split fills: more words than the canonical form, the same rows (test_encoders_decode_to_the_shape)
    assert len(words("split_fills")) > len(canon)


def test_path_census(encoded):
    hit = set()
    for (kind, variant, name, side), data in encoded.items():
        if kind == "concise":
            w = BV.concise_words(data)
            nw = len(w)
            hit.add("concise wave" if nw <= CONCISE_WAVE_WORDS else
                    "concise workgroup" if nw <= CONCISE_SPLIT_WORDS else "concise pieces")
            fill, one = (w >> 31) == 0, ((w >> 30) & 1) == 1
            flip = ((w >> 25) & 0x1F) > 0
            if (fill & one & flip).any():
                hit.add("one-fill with flip bit")
            if (fill & ~one & flip).any():
                hit.add("zero-fill with flip bit")
            if (fill & one & (31 * ((w & 0x01FFFFFF).astype(np.int64) + 1) > SEARCH_SHORT_ROWS)).any():
                hit.add("long one-fill")
        else:
            lay = BV.roaring_layout(data)
            kinds = {c[2] for c in lay["containers"]}
            if len(data) <= ROARING_SPLIT_BYTES:
                hit.add("roaring whole")
                hit.update(f"whole {k}" for k in kinds)
            else:
                hit.add("roaring pieces")
                hit.update(f"piece {k}" for k in kinds)
            n = len(lay["containers"])
            if lay["run_cookie"]:
                assert lay["offsets"] == (n >= 4)
                hit.add("run cookie, 3 containers" if n == 3 else "run cookie, 4 or more" if n >= 4 else "run cookie, 1 or 2")
            if any(c[3] > SEARCH_SHORT_ROWS for c in lay["containers"]):
                hit.add("long run")
            if any(c[1] == 65536 for c in lay["containers"]):
                hit.add(f"full container as {[c[2] for c in lay['containers'] if c[1] == 65536][0]}")
            for card in (4096, 4097):
                hit.update(f"cardinality {card} as {c[2]}" for c in lay["containers"] if c[1] == card)
            keys = [c[0] for c in lay["containers"]]
            if keys != list(range(keys[0], keys[0] + n)):
                hit.add("key gap")
    want = {"concise wave", "concise workgroup", "concise pieces", "one-fill with flip bit", "zero-fill with flip bit",
            "long one-fill", "roaring whole", "roaring pieces", "piece run", "piece array", "piece bitmap",
            "whole run", "whole array", "whole bitmap", "run cookie, 3 containers", "run cookie, 4 or more",
            "long run", "full container as run", "full container as bitmap", "cardinality 4096 as array",
            "cardinality 4096 as run", "cardinality 4097 as bitmap", "cardinality 4097 as run", "key gap"}
    assert want <= hit, sorted(want - hit)
    # the all-literal form of the density-0.5 shape is over the Concise split: 10,572 words
    assert len(encoded[("concise", "all_literal", "half", "in")]) // 4 == (BV.N_ROWS + 30) // 31 == 10_572


# ----------------------------------------------------------------------------------------------
# the compaction pairs
# ----------------------------------------------------------------------------------------------
def test_pairs_segment(O, W, kats, tmp_path):
    lists = BV.pair_lists(kats)
    assert len(lists) == 46
    seg = O.OracleSegment(BV.write_pairs_segment(W, str(tmp_path / "pairs"), kats))
    assert seg.dictionary("pairs") == [n for n, _ in lists] and seg.num_rows == BV.PAIR_ROWS
    for k, (name, words) in enumerate(lists):
        want = O.concise_rows(BV._be(words))
        assert len(want) and want[-1] < BV.PAIR_ROWS
        assert np.array_equal(seg.bitmap_rows("pairs", k), want), name
        if k % 2:
            assert np.array_equal(want, seg.bitmap_rows("pairs", k - 1)), name


# ----------------------------------------------------------------------------------------------
# the writer hook
# ----------------------------------------------------------------------------------------------
# sha256 of 00000.smoosh of _small_spec written without the hook, taken before the hook existed
DEFAULT_BYTES = {"concise": "6b4773e72e5c3e5d79797f12571e477a5d3efd91385f2af761006ffb582f18c1",
                 "roaring": "3893414a5777a3350cc8d21441617a297406eabc6d693439998eb9bb37573861"}


def _small_spec(W):
    n = 3000
    r = np.arange(n)
    tags = W.encode_multi_strings([["a", "b"][: i % 3] + ["t%d" % (i % 5)] if i % 11 else [] for i in range(n)])
    return W.SegmentSpec(timestamps=r.astype(np.int64) * 10,
                         dims={"d": W.encode_strings(["v%02d" % (i * i % 23) for i in range(n)]),
                               "run": W.encode_strings(np.where((r > 100) & (r < 2900), "x", "y").tolist()),
                               "tags": tags},
                         metrics={"m": ("long", r % 13)}, interval=(0, 10 * n))


def _smoosh(path):
    with open(os.path.join(path, "00000.smoosh"), "rb") as f:
        return f.read()


@pytest.mark.parametrize("kind", ["concise", "roaring"])
def test_hook_keeps_the_default_bytes(W, tmp_path, kind):
    spec = _small_spec(W)
    plain = _smoosh(W.write_segment(str(tmp_path / "plain"), spec, bitmap=kind))
    assert hashlib.sha256(plain).hexdigest() == DEFAULT_BYTES[kind]
    none = _smoosh(W.write_segment(str(tmp_path / "none"), spec, bitmap=kind, bitmap_encoder=None))
    assert none == plain
    # the canonical encoder through the hook: the same file, so the hook reaches every bitmap of single-
    # and multi-value columns with the value's rows
    calls = []

    def enc(rows, num_rows):
        assert rows.dtype == np.int64 and np.all(np.diff(rows) > 0) and num_rows == 3000
        calls.append(len(rows))
        return BV.ENCODERS[kind]["canonical"](rows, num_rows)

    hooked = _smoosh(W.write_segment(str(tmp_path / "hooked"), spec, bitmap=kind, bitmap_encoder=enc))
    assert hooked == plain
    assert len(calls) == sum(len(d[0]) for d in spec.dims.values())
    # and other bytes when the encoder gives other bytes
    other = _smoosh(W.write_segment(str(tmp_path / "other"), spec, bitmap=kind,
                                    bitmap_encoder=BV.ENCODERS[kind]["all_literal" if kind == "concise" else "all_run"]))
    assert other != plain and len(other) > len(plain)
