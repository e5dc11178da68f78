# Pages for the Snappy write-side tests (test_snappy_write_cpu.py,
# test_snappy_write_gpu.py and, through a file, the stand-alone check program
# snappy_compress_check). Everything is built from fixed seeds, so the CPU
# and GPU tests and the check program see the same bytes.
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), "tools"))
from gen_ssts import make_series_ids  # noqa: E402

LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 67, 68, 4095, 65536, 65544, 200000]
PERIODS = [2, 3, 8, 16, 64, 72]
LITERALS = [60, 61, 256, 257, 65536]
MATCHES = [4, 11, 12, 64, 65, 67, 68, 129]
DISTANCES = [65535, 65536, 65537]
ALIGNS = [0, 1, 7, 8, 63]
ROWS = 8192


def _rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _rand_unique(rng, n):
    """Random bytes in which no 4-byte window occurs twice, so that the only
    matches in a page are the ones its shape puts there."""
    while True:
        b = rng.integers(0, 256, n, dtype=np.uint8)
        if n < 5:
            return b.tobytes()
        w = (b[:-3].astype(np.uint32) | b[1:-2].astype(np.uint32) << 8 |
             b[2:-1].astype(np.uint32) << 16 | b[3:].astype(np.uint32) << 24)
        if len(np.unique(w)) == len(w):
            return b.tobytes()


def parse(stream):
    """A Snappy stream as (uncompressed length, elements): ("L", length) or
    ("C", offset, length, tag form 1 or 2)."""
    pos = ulen = shift = 0
    while True:
        b = stream[pos]
        pos += 1
        ulen |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    out = []
    while pos < len(stream):
        tag = stream[pos]
        pos += 1
        if tag & 3 == 0:
            n = (tag >> 2) + 1
            if n > 60:
                nb = n - 60
                n = int.from_bytes(stream[pos:pos + nb], "little") + 1
                pos += nb
            out.append(("L", n))
            pos += n
        elif tag & 3 == 1:
            out.append(("C", (tag >> 5) << 8 | stream[pos],
                        4 + ((tag >> 2) & 7), 1))
            pos += 1
        else:
            assert tag & 3 == 2, "4-byte-offset copies are never emitted"
            out.append(("C", int.from_bytes(stream[pos:pos + 2], "little"),
                        (tag >> 2) + 1, 2))
            pos += 2
    assert pos == len(stream)
    return ulen, out


def copy_elements(offset, length):
    """What Snappy's EmitCopy makes of one match."""
    out = []
    while length >= 68:
        out.append(("C", offset, 64, 2))
        length -= 64
    if length > 64:
        out.append(("C", offset, 60, 2))
        length -= 60
    out.append(("C", offset, length,
                1 if length < 12 and offset < 2048 else 2))
    return out


ZERO_GAPS = (98, 2998)      # match offsets M + 100 and M + 3000


def snappy_hash(w):
    return ((w * 0x1E35A7BD) & 0xFFFFFFFF) >> 20


def colliding_words():
    """Two different 4-byte words with the compressor's hash equal."""
    w1 = struct.unpack("<I", b"hxA1")[0]
    w2 = w1 + 1
    while snappy_hash(w2) != snappy_hash(w1):
        w2 += 1
    return struct.pack("<I", w1), struct.pack("<I", w2)


def metric_pages():
    """One 8192-row page per metric page class: (name, bytes, kind), kind in
    keys / values (the reference-encoder bar applies to keys only)."""
    rng = np.random.default_rng(20240917)
    out = []
    for k in (1, 2, 8, 100):
        ids = make_series_ids((ROWS + k - 1) // k, 7)
        out.append((f"series/{k}", np.repeat(ids, k)[:ROWS].tobytes(), "keys"))
    for k in (1, 2, 8, 100):
        ts = 1_700_000_000_000 + (np.arange(ROWS, dtype=np.int64) % k) * 10_000
        out.append((f"ts/{k}", ts.tobytes(), "keys"))
    out.append(("const_u64", np.full(ROWS, 12345, np.uint64).tobytes(),
                "keys"))
    out.append(("zeros", np.zeros(ROWS, np.uint64).tobytes(), "keys"))
    out.append(("f64_random", rng.random(ROWS).tobytes(), "values"))
    out.append(("f64_2dec", np.round(rng.random(ROWS) * 100, 2).tobytes(),
                "values"))
    out.append(("f64_small_int",
                rng.integers(0, 100, ROWS).astype(np.float64).tobytes(),
                "values"))
    return out


def shape_pages():
    """The hook list: (name, bytes) for every shape the issue names."""
    rng = np.random.default_rng(1234567)
    pages = []
    # lengths, over a low-entropy content (matches of every kind) and a
    # random one (nothing but literals)
    for n in LENGTHS:
        pages.append((f"len{n}/low",
                      rng.integers(0, 3, n, dtype=np.uint8).tobytes()))
        pages.append((f"len{n}/rand", _rand(rng, n)))
    # a constant byte and short periods, at a length that is no multiple of
    # the period or of 64
    pages.append(("const_byte", b"\x5a" * 5003))
    for per in PERIODS:
        blk = _rand(rng, per)
        pages.append((f"period{per}", (blk * (5003 // per + 1))[:5003]))
    # a match that ends at the last byte, and 1..3 bytes before it
    head = _rand(rng, 300)
    for tail in range(4):
        pages.append((f"match_end-{tail}",
                      head + head[10:110] + bytes([1, 2, 3][:tail])))
    # literals of every length form in front of a match (distance 32); the
    # literal holds no 4-byte window twice, so nothing splits it
    for k in LITERALS:
        lit = _rand_unique(rng, k)
        pages.append((f"literal{k}", lit + lit[-32:]))
    # copy lengths at the element boundaries, offset below and above 2048.
    # The gap between the two blocks is a zero run: it leaves as one short-
    # offset copy and inserts a handful of positions, so the block's table
    # entry survives it (random filler would evict it)
    for m in MATCHES:
        for zeros in ZERO_GAPS:
            body = _rand_unique(rng, 40 + m + 20)
            blk = body[40:40 + m]
            pages.append((f"match{m}/off{m + zeros + 2}",
                          body[:40] + b"\x33" + blk + b"\x11" +
                          b"\0" * zeros + b"\x44" + blk + b"\x22" +
                          body[40 + m:]))
    # a repeat at the offset limit and just past it; the zeros in between
    # are one long copy, so the block's table entries survive
    for d in DISTANCES:
        blk = _rand(rng, 32)
        pages.append((f"distance{d}",
                      blk + b"\0" * (d - 32) + blk + _rand(rng, 8)))
    # two words with one hash: the later one owns the table entry
    w1, w2 = colliding_words()
    t1, t2 = _rand(rng, 12), _rand(rng, 12)
    pages.append(("collide/12", _rand(rng, 50) + w1 + t1 + _rand(rng, 50) +
                  w2 + t2 + _rand(rng, 50) + w1 + t1 + _rand(rng, 9)))
    pages.append(("collide/21", _rand(rng, 50) + w2 + t2 + _rand(rng, 50) +
                  w1 + t1 + _rand(rng, 50) + w1 + t1 + _rand(rng, 9)))
    pages += [(name, page) for name, page, _ in metric_pages()]
    return pages


def pinned_elements():
    """name -> check(elements): what the streams of the constructed shapes
    must hold, so that the shapes keep producing the element forms they are
    there for. elements is parse(stream)[1]."""
    pins = {}

    def literal_then_copy(k):
        def check(el):
            assert el == [("L", k), ("C", 32, 32, 2)], el
        return check

    def one_far_match(m, offset):
        def check(el):
            want = copy_elements(offset, m)
            at = [i for i, e in enumerate(el) if e[0] == "C" and e[1] == offset]
            assert [el[i] for i in at] == want, (el, want)
            assert at == list(range(at[0], at[0] + len(want))), el
            assert el[at[0] - 1][0] == "L" and el[at[-1] + 1][0] == "L", el
            # every other copy belongs to the zero run
            assert all(e[1] <= 64 for i, e in enumerate(el)
                       if e[0] == "C" and i not in at), el
        return check

    def distance(d):
        def check(el):
            far = [e for e in el if e[0] == "C" and e[1] > 64]
            if d <= 65535:
                assert far == [("C", d, 32, 2)], far
            else:
                assert far == [], far
        return check

    for k in LITERALS:
        pins[f"literal{k}"] = literal_then_copy(k)
    for m in MATCHES:
        for zeros in ZERO_GAPS:
            pins[f"match{m}/off{m + zeros + 2}"] = one_far_match(
                m, m + zeros + 2)
    for d in DISTANCES:
        pins[f"distance{d}"] = distance(d)
    return pins


def dump(path, pages):
    """The file format snappy_compress_check reads."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(pages)))
        for _, page in pages:
            f.write(struct.pack("<I", len(page)))
            f.write(page)
