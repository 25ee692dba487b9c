"""Other legal LZF streams than the writer's (test side, plain Python and numpy).

The engine's LZF decoder (k_lzf_decode, incubator-druid_amd/csrc/dg_kernels.hip) is otherwise fed only what
dgt_lzf_compress writes: greedy matches, one hash table per chunk, chunks of 65535 + 1 bytes. This module
builds streams of the same published format (compress-lzf 1.0.4: "ZV" chunks, type 0 raw = u16 BE length +
bytes, type 1 = u16 BE compressed length + u16 BE plain length + liblzf tokens; a token is ctrl < 32 ->
ctrl + 1 literal bytes, else a back-reference of length (ctrl >> 5) + 2, 7 extended by the next byte, at
distance ((ctrl & 31) << 8 | next byte) + 1) token by token:

* scripts: lists of literal / reference / raw-chunk / chunk-cut ops. Script builds the stream and, byte by
  byte from the ops alone, the plaintext it must decode to. Every script is one full 65536-byte block of an
  8-byte long metric column (any 8 bytes are a legal value).
* re-encoders of given plaintext (all_literal, raw_only, pieces, alternating) for columns whose bytes are
  constrained: dictionary ids, packed longs, floats, __time.
* walk(): the kernel's window staging rule restated, to say at which window position every token and chunk
  header of a stream starts.
* malformed(): streams the decoder must refuse.

write_segment(..., lzf_encoder=hook) carries the streams through the real path."""
import copy
import functools
import importlib

import numpy as np

BLOCK = 65536
# k_lzf_decode's input window (dg_kernels.hip: kLzfWin = 8192; refill(): "if (ip + 48 <= we || we >= n) return;
# wb = ip & ~3; we = min(n, wb + kLzfWin)", called before every chunk header and every token)
WIN = 8192
MARGIN = 48
DISTANCES = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 8191, 8192)


def _tools():
    return importlib.import_module("incubator-druid_amd._tools")


# ------------------------------------------------------------------------------------------------
# tokens and chunks
# ------------------------------------------------------------------------------------------------
def _u16(v):
    assert 0 <= v <= 0xFFFF, v
    return bytes([v >> 8, v & 0xFF])


def lit(data):
    """A literal run of 1..32 bytes: ctrl = length - 1, then the bytes."""
    assert 1 <= len(data) <= 32
    return bytes([len(data) - 1]) + bytes(data)


def ref(dist, length):
    """A back-reference: 2 bytes for lengths 3..8, 3 bytes (ctrl 0xE0 | hi, length - 9, lo) for 9..264."""
    assert 1 <= dist <= 8192 and 3 <= length <= 264
    hi, lo = (dist - 1) >> 8, (dist - 1) & 0xFF
    if length <= 8:
        return bytes([((length - 2) << 5) | hi, lo])
    return bytes([0xE0 | hi, length - 9, lo])


def chunk_raw(data):
    return b"ZV\x00" + _u16(len(data)) + bytes(data)


def chunk_lzf(tokens, ulen):
    body = b"".join(tokens)
    return b"ZV\x01" + _u16(len(body)) + _u16(ulen) + body


# ------------------------------------------------------------------------------------------------
# scripts
# ------------------------------------------------------------------------------------------------
class Script:
    """Builds a stream op by op and, independently of any decoder, its plaintext. Records every token and
    chunk header (`events`: kind, stream offset ip, output offset op, ...) and every chunk (`chunks`).
    A type-1 chunk is cut by itself when one more token could overflow a u16 length."""

    def __init__(self, name, seed):
        self.name = name
        self.rng = np.random.default_rng(seed)
        self.plain = bytearray()
        self.stream = bytearray()
        self.events = []
        self.chunks = []
        self._hdr = None  # stream offset of the open type-1 chunk's header
        self._chunk_op = 0
        self._chunk_first = 0
        self.we = 0  # the window's end while building (as if the stream never ended)

    @property
    def pos(self):
        return len(self.stream)

    @property
    def op(self):
        return len(self.plain)

    def rand(self, n):
        return self.rng.integers(1, 256, n, dtype=np.uint8).tobytes()  # never 0: a read of zero padding shows

    def rep(self, n):
        """n compressible bytes (period 97): the writer's encoder would not store them raw."""
        return (self.rand(97) * (n // 97 + 1))[:n]

    def _event(self, kind, **info):
        if self.pos + MARGIN > self.we:
            self.we = (self.pos & ~3) + WIN
        self.events.append(dict(kind=kind, ip=self.pos, op=self.op, **info))

    def _open(self, need_body, need_plain):
        if self._hdr is not None and (self.pos - self._hdr - 7 + need_body > 0xFFFF or
                                      self.op - self._chunk_op + need_plain > 0xFFFF):
            self.cut()
        if self._hdr is None:
            self._event("hdr7")
            self._hdr, self._chunk_op, self._chunk_first = self.pos, self.op, len(self.events)
            self.stream += bytes(7)

    def cut(self):
        """End the open type-1 chunk (no-op when none is open)."""
        if self._hdr is None:
            return
        h, body, ulen = self._hdr, self.pos - self._hdr - 7, self.op - self._chunk_op
        assert body > 0 and ulen > 0
        self.stream[h:h + 7] = b"ZV\x01" + _u16(body) + _u16(ulen)
        toks = self.events[self._chunk_first:]
        self.chunks.append(dict(type=1, plain=ulen, comp=body,
                                only_lit32=all(t["kind"] == "lit" and t["n"] == 32 for t in toks)))
        self._hdr = None

    def lit(self, data):
        self._open(1 + len(data), len(data))
        self._event("lit", n=len(data))
        self.stream += lit(data)
        self.plain += data

    def ref(self, dist, length):
        self._open(3, length)
        assert dist <= self.op, (self.name, dist, self.op)
        self._event("ref2" if length <= 8 else "ref3", dist=dist, n=length, chunk_op=self._chunk_op)
        self.stream += ref(dist, length)
        for _ in range(length):  # byte by byte: an overlapping reference repeats itself
            self.plain.append(self.plain[len(self.plain) - dist])

    def raw(self, data):
        self.cut()
        self._event("hdr5", n=len(data))
        self.stream += chunk_raw(data)
        self.plain += data
        self.chunks.append(dict(type=0, plain=len(data), comp=len(data), only_lit32=False))

    def lits(self, n):
        """n random bytes as 32-byte literal runs and one shorter run."""
        while n > 0:
            k = min(n, 32)
            self.lit(self.rand(k))
            n -= k

    def fill_stream(self, g):
        """Literal tokens that take exactly g stream bytes (each 2..33)."""
        assert g == 0 or g >= 2, g
        while g > 0:
            t = g if g <= 33 else (32 if g - 33 == 1 else 33)
            self.lit(self.rand(t - 1))
            g -= t

    def approach(self, s):
        """Literal tokens up to stream offset we - s, none of which restages the window: each starts at or
        before we - 48, so the last one spans from there to we - s (s >= 15: a token has at most 33 bytes)."""
        assert 15 <= s <= MARGIN
        self._open(1 + 32, 32)
        if self.pos + MARGIN > self.we:  # the token here restages: let it, then count from the new window
            self.lit(self.rand(32))
        last = max(MARGIN - s, 2)
        while self.we - s - last - self.pos < 0 or self.we - s - last - self.pos == 1:  # too near: the next window
            self.lit(self.rand(32))
        self.fill_stream(self.we - s - last - self.pos)
        self.fill_stream(last)
        assert self.pos == self.we - s and self._hdr is not None

    def close(self, end=None, mod4=None):
        """Pad the plaintext to BLOCK with literal runs. end: "lit32" / "ref264", the last token, ending exactly
        at BLOCK. mod4: the stream length's residue, set by splitting up to three runs in two."""
        if mod4 is not None:
            for k in range(8):
                t = copy.deepcopy(self)
                t._close(end, k)
                if len(t.stream) % 4 == mod4:
                    self.__dict__.update(t.__dict__)
                    return self
            raise AssertionError(f"{self.name}: no split gives n % 4 == {mod4}")
        self._close(end, 0)
        return self

    def _close(self, end, splits):
        final = {None: 0, "lit32": 32, "ref264": 264}[end]
        r = BLOCK - self.op - final
        assert r >= 0 and (r >= 32 * splits + 32 or splits == 0), (self.name, r)
        self.lits(r - r % 32 - 32 * splits)
        for _ in range(splits):
            self.lit(self.rand(16))
            self.lit(self.rand(16))
        if r % 32:
            self.lit(self.rand(r % 32))
        if end == "lit32":
            self.lit(self.rand(32))
        elif end == "ref264":
            self.ref(777, 264)
        self.cut()
        assert self.op == BLOCK, (self.name, self.op)


def _lengths():
    """Every literal run length and every reference length, over the distance list; the first reference
    reaches output byte 0 (dist == op). Ends with a 32-byte literal run at exactly BLOCK."""
    s = Script("lengths", 1)
    s.lit(s.rand(5))
    s.ref(5, 5)
    for n in range(1, 33):
        s.lit(s.rand(n))
    s.lits(8192)
    for i, length in enumerate(range(3, 265)):
        s.ref(DISTANCES[i % len(DISTANCES)], length)
        s.lit(s.rand(1 + (i * 7) % 32))
    return s.close("lit32", 0)


OVERLAPS = {"dist < length <= 64": [(5, 40), (3, 64), (63, 64)],
            "dist < length, length > 64": [(7, 200), (2, 65), (63, 129)],
            "64 < dist < length": [(100, 250), (65, 264), (65, 66)],
            "dist == length": [(3, 3), (10, 10), (64, 64), (65, 65), (200, 200), (264, 264)],
            "length == 2 * dist + 1": [(1, 3), (20, 41), (64, 129), (100, 201)],
            "dist == 1 at length 264": [(1, 264)]}


def _overlaps():
    """The overlap classes, references into the previous chunk's output (distance is measured from the
    block's start in both of our decoders), every distance at long and short lengths. Ends with a
    264-byte reference at exactly BLOCK."""
    s = Script("overlaps", 2)
    s.lits(300)
    for cases in OVERLAPS.values():
        for dist, length in cases:
            s.lit(s.rand(7))
            s.ref(dist, length)
    s.lits(40)
    s.cut()
    s.ref(50, 30)      # the first token of a chunk, wholly inside the previous chunk's output
    s.lit(s.rand(3))
    s.ref(40, 264)     # starts in the previous chunk's output, runs into this chunk's
    s.lits(8192)
    s.cut()
    s.ref(8192, 100)   # the farthest distance, across a chunk boundary
    for d in DISTANCES:
        s.lit(s.rand(9))
        s.ref(d, 3)
        s.lit(s.rand(2))
        s.ref(d, 8)
        s.ref(d, 9)
        s.lit(s.rand(31))
        s.ref(d, 264)
    return s.close("ref264", 1)


def _small_chunks():
    """Hundreds of chunks of 1, 2, 3, 5 and a few more bytes, raw and type 1 in turn: the next header starts
    at every address residue, raw chunks end inside the window with type-1 tokens right after them."""
    s = Script("small_chunks", 3)
    for i in range(90):
        for k in (1, 2, 3, 5):
            s.raw(s.rand(k))
            if (i + k) % 2:
                s.lit(s.rand(1 + (i + k) % 2))   # a type-1 chunk of 1 or 2 bytes
                s.cut()
        s.lit(s.rand(1))
        s.cut()
        s.lit(s.rand(2))
        s.cut()
        s.lit(s.rand(4 + i % 9))
        s.ref(1 + i % 11, 3 + i % 30)
        s.cut()
    return s.close("lit32", 2)


def _raw_65535():
    s = Script("raw_65535", 4)
    s.raw(s.rep(65535))
    s.raw(s.rand(1))
    return s.close()


def _raw_halves():
    s = Script("raw_halves", 5)
    s.raw(s.rep(32768))
    s.raw(s.rep(32768))
    return s.close()


def _literal_halves():
    """Two type-1 chunks of 32768 bytes made only of 32-byte literal runs: the stream is longer than the block."""
    s = Script("literal_halves", 6)
    s.lits(32768)
    s.cut()
    s.lits(32768)
    return s.close()


def _lzf_65535():
    """A type-1 chunk of 65535 plaintext bytes (it needs references to fit a u16 compressed length), then one of 1."""
    s = Script("lzf_65535", 7)
    for _ in range(221):
        s.lit(s.rand(32))
        s.ref(32, 264)
    s.lits(65535 - s.op)
    assert s.op == 65535 and len(s.chunks) == 0
    s.cut()
    s.lit(s.rand(1))
    return s.close()


def _literal_63520():
    """The largest type-1 chunk made only of 32-byte literal runs (63,520 bytes, 65,505 compressed), a chunk
    of 2 bytes, then the rest."""
    s = Script("literal_63520", 8)
    s.lits(63520)
    s.cut()
    s.lit(s.rand(2))
    s.cut()
    return s.close("lit32", 3)


def _lead(k):
    """A lead literal of k bytes, then 32-byte runs: token starts sweep the end of the first window."""
    s = Script(f"lead{k:02d}", 100 + k)
    s.lit(s.rand(k))
    return s.close("lit32" if k % 2 else None, k % 4)


# Window positions. A token can start at we - s without a restage before it only for s >= 15: the token before
# it started at or before we - 48 (or it would have restaged) and has at most 33 bytes. A chunk header can
# start anywhere, after a raw chunk. (A token nearer than 15 to the window's end exists only where the window
# ends with the stream, the `we >= n` return: the last tokens of every script.)
TOKEN_S = tuple(range(15, MARGIN + 1))
FEW_S = (15, 16, 17, 18, 47, 48)
HEADER_S = (1, 2, 3, 4, 5, 6, 7, 8, 47, 48)
PHASE_TARGETS = ([("lit33", s) for s in TOKEN_S] + [(k, s) for s in FEW_S for k in ("ref3", "ref2")] +
                 [(k, s) for s in HEADER_S for k in ("hdr7", "hdr5")])
PHASES_PER_BLOCK = 7


def _place(s, kind, at):
    if kind in ("hdr7", "hdr5"):
        s.cut()
        if s.pos + MARGIN > s.we:
            s.lit(s.rand(32))  # restages; the raw chunk's header must not
            s.cut()
        n = s.we - at - s.pos - 5
        assert n >= 1
        s.raw(s.rand(n))
        assert s.pos == s.we - at
        if kind == "hdr7":
            s.lit(s.rand(32))
        else:
            s.raw(s.rand(41))
        return
    s.approach(at)
    if kind == "lit33":
        s.lit(s.rand(32))
    elif kind == "ref3":
        s.ref(300 + at, 40)
    else:
        s.ref(70 + at, 5)


def _phases(i):
    s = Script(f"phases{i:02d}", 200 + i)
    s.lit(s.rand(1 + i % 32))
    for kind, at in PHASE_TARGETS[i * PHASES_PER_BLOCK:(i + 1) * PHASES_PER_BLOCK]:
        _place(s, kind, at)
    return s.close("ref264" if i % 8 >= 4 else "lit32", i % 4)


@functools.lru_cache(maxsize=None)
def scripts():
    """name -> closed Script (stream, plaintext, events, chunks), in a fixed order."""
    out = [_lengths(), _overlaps(), _small_chunks(), _raw_65535(), _raw_halves(), _literal_halves(), _lzf_65535(),
           _literal_63520()]
    out += [_lead(k) for k in range(1, 33)]
    out += [_phases(i) for i in range((len(PHASE_TARGETS) + PHASES_PER_BLOCK - 1) // PHASES_PER_BLOCK)]
    for s in out:
        assert len(s.plain) == BLOCK, s.name
    return {s.name: s for s in out}


def script_groups(k=4):
    """The script names in k groups of about equal size (one segment each in the GPU test)."""
    names = list(scripts())
    return [names[i::k] for i in range(k)]


def script_values(names):
    """The long column of the named scripts' blocks."""
    return np.frombuffer(b"".join(bytes(scripts()[n].plain) for n in names), dtype="<i8")


def script_hook(names):
    """lzf_encoder for write_segment: a script's plaintext -> its stream, anything else -> the build's encoder."""
    table = {bytes(scripts()[n].plain): bytes(scripts()[n].stream) for n in names}
    used = set()

    def hook(plain):
        if plain in table:
            used.add(plain)
            return table[plain]
        return _tools().lzf_compress(plain)

    hook.table, hook.used = table, used
    return hook


# ------------------------------------------------------------------------------------------------
# the window model
# ------------------------------------------------------------------------------------------------
def walk(script):
    """The kernel's staging rule over a script's stream (dg_kernels.hip, refill(): before each chunk header
    and each token, if ip + 48 > we and we < n then wb = ip & ~3, we = min(n, wb + 8192)). Per event:
    (kind, ip, s = we - ip before the rule, restaged, phase = (ip - wb) & 3 after it, at_end = we >= n)."""
    n = len(script.stream)
    wb = we = 0
    out = []
    for e in script.events:
        ip = e["ip"]
        s = we - ip
        restaged = ip + MARGIN > we and we < n
        if restaged:
            wb = ip & ~3
            we = min(n, wb + WIN)
        assert wb <= ip < we
        out.append(dict(e, s=s, restaged=restaged, phase=(ip - wb) & 3, at_end=we >= n, wb=wb, we=we))
    return out


# ------------------------------------------------------------------------------------------------
# re-encoders of given plaintext
# ------------------------------------------------------------------------------------------------
def _literal_chunk(data):
    assert 0 < len(data) <= 63520
    return chunk_lzf([lit(data[i:i + 32]) for i in range(0, len(data), 32)], len(data))


def all_literal(data):
    """Type-1 chunks of literal runs only."""
    return b"".join(_literal_chunk(data[i:i + 63520]) for i in range(0, len(data), 63520))


def raw_only(sizes):
    """Raw chunks of the given sizes in turn."""
    def enc(data):
        out, i, k = [], 0, 0
        while i < len(data):
            out.append(chunk_raw(data[i:i + sizes[k % len(sizes)]]))
            i += sizes[k % len(sizes)]
            k += 1
        return b"".join(out)
    return enc


def pieces(k):
    """The build's encoder over k-byte pieces: many type-1 chunks, each with its own matches."""
    def enc(data):
        return b"".join(_tools().lzf_compress(data[i:i + k]) for i in range(0, len(data), k))
    return enc


def alternating(k):
    """k-byte pieces, in turn a raw chunk and a type-1 chunk (the build's where it compresses, else literal runs)."""
    def enc(data):
        out = []
        for j, i in enumerate(range(0, len(data), k)):
            piece = data[i:i + k]
            if j % 2 == 0:
                out.append(chunk_raw(piece))
            else:
                c = _tools().lzf_compress(piece)
                out.append(c if c[2] == 1 else _literal_chunk(piece))
        return b"".join(out)
    return enc


REENCODERS = {"all_literal": all_literal, "raw_only": raw_only([1, 2, 3, 5, 9000, 70]), "pieces": pieces(100),
              "alternating": alternating(333)}

# Row counts of the constrained-column segments: one block per column, and the last (only) block's decoded
# length leaves every remainder mod 16 the byte tail store has to write (see decoded_lengths).
CONSTRAINED_ROWS = (4093, 4097, 4111)


def decoded_lengths(n):
    """Decoded block length per column kind of an n-row, one-block segment (what k_lzf_decode writes out:
    ids are id_bytes wide, packed longs carry VSizeLongSerde's 4 closing bytes)."""
    return {"id1": n, "id2": 2 * n, "id3": 3 * n, "id4": 4 * n, "float": 4 * n, "long": 8 * n,
            "delta12": (12 * n + 7) // 8 + 4, "table4": (4 * n + 7) // 8 + 4}


def constrained_spec(W, n, packed):
    """packed: the DELTA (12 bit) and TABLE (4 bit) columns, to be written with long_encoding="auto";
    else ids, a float, a wide long and __time, with long_encoding="longs"."""
    rng = np.random.default_rng(n)
    ts = np.sort(rng.integers(10_000, 10_000 + 3 * 3_600_000, n)).astype(np.int64)
    dims = {"a": W.encode_int_strings(rng.integers(0, 200, n)), "b": W.encode_int_strings(rng.zipf(1.3, n) % 50)}
    if packed:
        metrics = {"delta": ("long", 1_000_000 + rng.integers(0, 4000, n)), "table": ("long", rng.integers(0, 9, n) * 1111)}
    else:
        metrics = {"wide": ("long", rng.integers(-(1 << 62), 1 << 62, n)), "f": ("float", rng.normal(3, 1, n).astype(np.float32))}
    return W.SegmentSpec(timestamps=ts, dims=dims, metrics=metrics)


# Row counts of the value-only segments (no dictionary ids): even, so the plain __time leaves no tail, and such
# that a 24-bit DELTA __time's tail holds none but VSizeLongSerde's closing bytes, while a float column (4122)
# and a 12-bit DELTA column leave tails of 8, 10, 11 and 12 bytes of values. What the byte tail store writes
# there is read as values only, never as an index.
VALUE_TAIL_ROWS = (4100, 4112, 4122)


def value_tail_spec(W, n, packed):
    rng = np.random.default_rng(n + 1)
    ts = np.sort(rng.integers(10_000, 10_000 + 3 * 3_600_000, n)).astype(np.int64)
    ts[0], ts[-1] = 10_000, 10_000 + 3 * 3_600_000 - 1  # a fixed range: 24 bits
    if packed:
        metrics = {"delta": ("long", 1_000_000 + rng.integers(0, 4000, n))}
    else:
        metrics = {"f": ("float", rng.normal(3, 1, n).astype(np.float32))}
    return W.SegmentSpec(timestamps=ts, metrics=metrics)


def recording(enc):
    """enc, remembering (plaintext, stream) of every block it is asked for."""
    seen = []

    def hook(plain):
        out = enc(plain)
        seen.append((plain, out))
        return out

    hook.seen = seen
    return hook


# ------------------------------------------------------------------------------------------------
# malformed streams
# ------------------------------------------------------------------------------------------------
MALFORMED_ROWS = 8192


def malformed_values():
    return (np.arange(MALFORMED_ROWS, dtype=np.int64) * 0x0101010101 + 7).astype("<i8")


def malformed():
    """name -> stream that a decoder of the block malformed_values() (65536 bytes) must refuse. All but
    "short" are refused whatever length is expected; "short" is a well-formed stream of 65528 bytes."""
    plain = malformed_values().tobytes()
    good = pieces(30000)(plain)
    head = _literal_chunk(plain[:40000])
    r32 = bytes(range(1, 33))
    return {
        "bad magic": b"ZW" + good[2:],
        "chunk type 2": b"ZV\x02" + good[3:],
        "header cut at 4": good + b"ZV\x01\x00",
        "header cut at 6": good + b"ZV\x01\x00\x05\x00",
        "raw chunk past the stream": head + b"ZV\x00" + _u16(25536) + plain[40000:65535],
        "compressed length past the stream": head + b"ZV\x01" + _u16(100) + _u16(32) + lit(r32),
        "chunk past the block": head + _literal_chunk(plain[:40000]),
        "raw chunk past the block": head + chunk_raw(plain[:40000]),
        "literal run past the chunk": b"ZV\x01" + _u16(5) + _u16(32) + lit(r32) + good,
        "literal run past the plain length": b"ZV\x01" + _u16(33) + _u16(16) + lit(r32) + good,
        "short reference cut": chunk_lzf([lit(r32), b"\x20"], 35) + good,
        "long reference cut at its length": chunk_lzf([lit(r32), b"\xe0"], 41) + good,
        "long reference cut at its offset": chunk_lzf([lit(r32), b"\xe0\x00"], 41) + good,
        "distance op + 1": chunk_lzf([lit(r32[:5]), ref(6, 3)], 8) + good,
        "distance 8192 at op 10": chunk_lzf([lit(r32[:10]), ref(8192, 3)], 13) + good,
        "reference past the plain length": chunk_lzf([lit(r32), ref(4, 20)], 40) + good,
        "chunk ends before its plain length": chunk_lzf([lit(r32), ref(4, 18)], 100) + good,
        "3 trailing bytes": good + b"ZV\x00",
        "short": pieces(30000)(plain[:BLOCK - 8]),
    }
