# Snappy decode paths on the GPU.
#
# Part 1 drives the production decode launch directly through the
# hx_debug_snappy_decompress test hook with hand-built streams (pair runs,
# same-offset runs, what follows a direct-to-dst run, malformed streams, a
# mixed batch) and compares the output bytes exactly against this file's own
# element decoder, which is itself cross-checked against pyarrow once.
# Every parametrisation of one property goes into ONE launch.
#
# Part 2 goes through Store: stored (single-literal) pages must be read in
# place — decode_stats() has to agree with this file's own tag walker — and
# every result must match the oracle at the suite's bar (keys, counts, min,
# max exact; sums rtol 1e-9).
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from oracle.scan import AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX
from tools.gen_ssts import gen_dataset, gen_sst_from_arrays, middle_range

pytestmark = pytest.mark.gpu

OPS = AGG_SUM | AGG_COUNT | AGG_MIN | AGG_MAX


# ---------------------------------------------------------------------------
# a small Snappy element encoder / decoder (snappy format_description.txt)
# ---------------------------------------------------------------------------
def varint(v):
    o = bytearray()
    while v >= 0x80:
        o.append((v & 0x7F) | 0x80)
        v >>= 7
    o.append(v)
    return bytes(o)


def lit(data):
    n = len(data) - 1
    if n < 60:
        return bytes([n << 2]) + data
    nb = 1 if n < 1 << 8 else 2 if n < 1 << 16 else 3
    return bytes([(59 + nb) << 2]) + n.to_bytes(nb, "little") + data


def copy(off, ln, kind=None):
    if kind is None:
        kind = 1 if (4 <= ln <= 11 and off < 2048) else 2
    if kind == 1:
        assert 4 <= ln <= 11 and off < 2048
        return bytes([1 | ((ln - 4) << 2) | ((off >> 8) << 5), off & 0xFF])
    assert 1 <= ln <= 64 and off < 65536
    return bytes([2 | ((ln - 1) << 2)]) + off.to_bytes(2, "little")


def run(off, total):
    """`total` bytes of same-offset copies: 64-byte 2-byte-offset elements
    (the ts-page shape) plus one remainder element."""
    out = copy(off, 64, kind=2) * (total // 64)
    if total % 64:
        out += copy(off, total % 64, kind=2)
    return out


def pair(b7):
    """{lit7, copy off=8 len=9}: the 10-byte series-page pair."""
    return lit(b7) + copy(8, 9, kind=1)


def expand(body, limit=None):
    """Output of an element sequence (no preamble). Raises ValueError on a
    malformed element; stops once `limit` bytes are out."""
    pos, out = 0, bytearray()
    while pos < len(body) and (limit is None or len(out) < limit):
        tag = body[pos]
        kind = tag & 3
        if kind == 0:
            ln = (tag >> 2) + 1
            pos += 1
            if ln > 60:
                nb = ln - 60
                if pos + nb > len(body):
                    raise ValueError("literal header past end")
                ln = int.from_bytes(body[pos:pos + nb], "little") + 1
                pos += nb
            if pos + ln > len(body):
                raise ValueError("literal past end")
            out += body[pos:pos + ln]
            pos += ln
            continue
        hdr = (0, 2, 3, 5)[kind]
        if pos + hdr > len(body):
            raise ValueError("copy header past end")
        if kind == 1:
            ln = ((tag >> 2) & 7) + 4
            off = ((tag >> 5) << 8) | body[pos + 1]
        else:
            ln = (tag >> 2) + 1
            off = int.from_bytes(body[pos + 1:pos + hdr], "little")
        pos += hdr
        if off == 0 or off > len(out):
            raise ValueError("bad offset")
        if off >= ln:
            start = len(out) - off
            out += out[start:start + ln]
        else:
            pat = bytes(out[-off:])
            out += (pat * (ln // off + 1))[:ln]
    return bytes(out)


def decode(buf):
    """Reference decoder of a whole stream (preamble + elements)."""
    pos, ulen, sh = 0, 0, 0
    while True:
        if pos >= len(buf) or pos >= 5:
            raise ValueError("preamble")
        b = buf[pos]
        pos += 1
        ulen |= (b & 0x7F) << sh
        if not b & 0x80:
            break
        sh += 7
    out = expand(buf[pos:], limit=ulen)
    if len(out) != ulen:
        raise ValueError("length mismatch")
    return out


def build(elements):
    """(stream, expected output) of a well-formed element list."""
    body = b"".join(elements)
    out = expand(body)
    return varint(len(out)) + body, out


# ---------------------------------------------------------------------------
# the debug hook
# ---------------------------------------------------------------------------
def gpu_decode(streams, ulens):
    """One production decode launch over all streams. Returns (outputs,
    n_errors); outputs[i] has ulens[i] bytes."""
    from horaedb_amd import store as hx_store
    lib = hx_store._lib
    fn = lib.hx_debug_snappy_decompress
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                   C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    n = len(streams)
    blob = np.frombuffer(b"".join(streams), dtype=np.uint8).copy()
    clens = np.array([len(s) for s in streams], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(clens[:-1], dtype=np.uint64)
    ul = np.array(ulens, dtype=np.uint32)
    out_offs = np.zeros(n, dtype=np.uint64)
    out_offs[1:] = np.cumsum(ul[:-1], dtype=np.uint64)
    out = np.full(int(ul.sum()) + 1, 0xA5, dtype=np.uint8)
    nerr = C.c_uint64(0)
    rc = fn(blob.ctypes.data, offs.ctypes.data, clens.ctypes.data,
            ul.ctypes.data, n, out.ctypes.data, out_offs.ctypes.data,
            C.byref(nerr))
    assert rc == 0, lib.hx_last_error().decode()
    outs = [out[int(o):int(o) + int(u)].tobytes()
            for o, u in zip(out_offs, ul)]
    return outs, nerr.value


def check_exact(cases):
    """cases: list of (label, (stream, expected)). One launch, byte-exact
    outputs, zero errors."""
    assert all(len(e) <= 65536 for _, (_, e) in cases)
    outs, nerr = gpu_decode([s for _, (s, _) in cases],
                            [len(e) for _, (_, e) in cases])
    bad = [lbl for (lbl, (_, e)), o in zip(cases, outs) if o != e]
    assert nerr == 0, f"{nerr} streams rejected"
    assert not bad, f"{len(bad)} of {len(cases)} differ, first: {bad[:8]}"


def rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def pairs(rng, n):
    return [pair(rnd(rng, 7)) for _ in range(n)]


def test_reference_decoder_matches_pyarrow():
    import pyarrow as pa
    rng = np.random.default_rng(1)
    codec = pa.Codec("snappy")
    # pyarrow's compressor -> this decoder
    series = np.sort(np.repeat(
        rng.integers(0, 2**63, 3000, dtype=np.uint64), 2))
    ts = 1_700_000_000_000 + 10_000 * np.arange(8192, dtype=np.int64)
    for raw in (series.tobytes(), ts.tobytes(), rnd(rng, 65536),
                b"ab" * 700, bytes(300)):
        assert decode(codec.compress(raw, asbytes=True)) == raw
    # this encoder -> pyarrow's decompressor
    s, raw = build([lit(rnd(rng, 8))] + pairs(rng, 70) +
                   [lit(rnd(rng, 5)), run(16, 700), lit(rnd(rng, 300)),
                    copy(900, 33), run(1, 100), copy(2047, 11, kind=1)])
    assert codec.decompress(s, decompressed_size=len(raw),
                            asbytes=True) == raw


# ---------------------------------------------------------------------------
# pair runs
# ---------------------------------------------------------------------------
def test_pair_runs_every_alignment():
    rng = np.random.default_rng(2)
    cases = []
    for n in (1, 63, 64, 65, 130, 4095):
        for lead in range(1, 17):  # run starts at d = lead: every d mod 16
            cases.append((f"pairs={n} lead={lead}",
                          build([lit(rnd(rng, lead))] + pairs(rng, n))))
    # 4095 pairs after a 16-byte lead-in end exactly at 64 KB
    assert len(cases[-1][1][1]) == 65536
    check_exact(cases)


def test_pair_runs_broken_and_followed():
    rng = np.random.default_rng(3)
    cases = []
    for lead in (3, 8, 16):
        for n0, n1 in ((10, 10), (64, 64), (100, 200), (63, 1)):
            # off=8 len=10 instead of len=9: same tags but the third byte
            brk10 = lit(rnd(rng, 7)) + copy(8, 10, kind=1)
            # a 6-byte literal where the 7-byte one is expected
            brk6 = lit(rnd(rng, 6)) + copy(8, 9, kind=1)
            for name, brk in (("len10", brk10), ("lit6", brk6)):
                cases.append((f"{name} lead={lead} {n0}+{n1}", build(
                    [lit(rnd(rng, lead))] + pairs(rng, n0) + [brk] +
                    pairs(rng, n1) + [lit(rnd(rng, 3))])))
    check_exact(cases)


def test_pair_run_truncated_by_comp_len():
    rng = np.random.default_rng(4)
    good_s, good = build([lit(rnd(rng, 8))] + pairs(rng, 65))
    streams, ulens = [], []
    # the 65th pair cut at every byte: the stream is short of its preamble
    for cut in range(1, 10):
        streams.append(good_s[:len(good_s) - cut])
        ulens.append(len(good))
    streams.append(good_s)
    ulens.append(len(good))
    outs, nerr = gpu_decode(streams, ulens)
    assert nerr == 9
    assert outs[-1] == good


# ---------------------------------------------------------------------------
# same-offset runs
# ---------------------------------------------------------------------------
def test_same_offset_runs_every_alignment():
    rng = np.random.default_rng(5)
    cases = []
    for off in (1, 2, 4, 8, 16, 24, 32):
        for k in range(1, 17):
            lead = 32 + k  # >= off, and the run starts at every d mod 16
            for total in (64, 4096, 65528 - lead, 65536 - lead):
                cases.append((f"off={off} lead={lead} run={total}",
                              build([lit(rnd(rng, lead)), run(off, total)])))
    check_exact(cases)


def test_same_offset_runs_mixed_element_sizes():
    # fused chains made of 1-byte- and 2-byte-offset elements of odd sizes
    rng = np.random.default_rng(6)
    cases = []
    for off in (1, 2, 4, 8, 16, 3, 12):
        for lead in (16, 21, 24, 31):
            els = [lit(rnd(rng, lead))]
            for _ in range(60):
                ln = int(rng.integers(1, 65))
                els.append(copy(off, ln))
            els.append(lit(rnd(rng, 9)))
            cases.append((f"off={off} lead={lead}", build(els)))
    check_exact(cases)


# ---------------------------------------------------------------------------
# what follows a direct run: the ring mirror and the register tail
# ---------------------------------------------------------------------------
def test_elements_after_direct_runs():
    rng = np.random.default_rng(7)
    runs = {
        "pairs": lambda: pairs(rng, 400),            # 6400 bytes
        "off8": lambda: [run(8, 6400)],
        "off16": lambda: [run(16, 6403)],
        "off1": lambda: [run(1, 6001)],
        "pairs-short": lambda: pairs(rng, 70),
        "off8-short": lambda: [run(8, 300)],
    }
    cases = []
    for rname, mk in runs.items():
        for lead in (8, 16, 19):
            head = [lit(rnd(rng, 16)), lit(rnd(rng, lead))]
            produced = len(expand(b"".join(head + mk())))
            afters = {f"copy{o}": [copy(o, 37)]
                      for o in (1, 8, 2047, 2049, 4095, 5000)
                      if o <= produced}
            afters["copy2047k1"] = [copy(2047, 11, kind=1)] \
                if produced >= 2047 else [copy(9, 11, kind=1)]
            afters["tiny"] = [lit(rnd(rng, 3))]
            afters["lit4096"] = [lit(rnd(rng, 4096))]
            afters["lit5001"] = [lit(rnd(rng, 5001))]
            for aname, after in afters.items():
                tail = [lit(rnd(rng, 5)), copy(8, 12), lit(rnd(rng, 8))] + \
                    pairs(rng, 5) + [copy(16, 40), copy(3000, 64)
                                     if produced >= 3000 else copy(7, 64)]
                cases.append((f"{rname} lead={lead} then {aname}",
                              build(head + mk() + after + tail)))
    check_exact(cases)


# ---------------------------------------------------------------------------
# malformed streams
# ---------------------------------------------------------------------------
def test_malformed_streams_counted_and_isolated():
    rng = np.random.default_rng(8)
    good = [build([lit(rnd(rng, 8))] + pairs(rng, 100)),
            build([lit(rnd(rng, 16)), run(8, 5000)]),
            build([lit(rnd(rng, 40))])]
    bad = [
        # copy offset greater than d
        (varint(8) + lit(rnd(rng, 4)) + copy(9, 4), 8),
        # ... after a direct run
        (varint(4200) + lit(rnd(rng, 8)) + run(8, 4096) + copy(4200, 64)
         + copy(8, 32), 4200),
        # literal runs past comp_len
        (varint(100) + lit(rnd(rng, 100))[:52], 100),
        # output short of uncomp_len
        (varint(100) + lit(rnd(rng, 50)), 100),
        # same-offset run longer than uncomp_len
        (varint(1000) + lit(rnd(rng, 8)) + run(8, 1024), 1000),
        # pair run longer than uncomp_len
        (varint(8 + 16 * 70 - 3) + lit(rnd(rng, 8)) +
         b"".join(pairs(rng, 70)), 8 + 16 * 70 - 3),
    ]
    for s, _ in bad:
        with pytest.raises(ValueError):
            decode(s)
    streams = [good[0][0], bad[0][0], bad[1][0], good[1][0], bad[2][0],
               bad[3][0], bad[4][0], good[2][0], bad[5][0]]
    ulens = [len(good[0][1]), bad[0][1], bad[1][1], len(good[1][1]),
             bad[2][1], bad[3][1], bad[4][1], len(good[2][1]), bad[5][1]]
    outs, nerr = gpu_decode(streams, ulens)
    assert nerr == len(bad)
    assert outs[0] == good[0][1]
    assert outs[3] == good[1][1]
    assert outs[7] == good[2][1]


# ---------------------------------------------------------------------------
# a mixed batch: waves take different paths side by side
# ---------------------------------------------------------------------------
def test_batch_of_mixed_streams():
    rng = np.random.default_rng(9)
    cases = []
    for i in range(300):
        els = [lit(rnd(rng, int(rng.integers(1, 40))))]
        produced = len(els[0]) - 1
        for _ in range(int(rng.integers(1, 12))):
            kind = int(rng.integers(0, 6))
            room = 65536 - produced
            if room < 6000:
                break
            if kind == 0:
                n = int(rng.integers(1, 200))
                els += pairs(rng, n)
                produced += 16 * n
            elif kind == 1:
                off = int(rng.choice([1, 2, 4, 8, 16, 24]))
                if off > produced:
                    continue
                n = int(rng.integers(1, 5000))
                els.append(run(off, n))
                produced += n
            elif kind == 2:
                n = int(rng.choice([1, 5, 7, 8, 59, 60, 61, 300, 4096, 4500]))
                els.append(lit(rnd(rng, n)))
                produced += n
            elif kind == 3:
                off = int(rng.integers(1, min(produced, 65535) + 1))
                n = int(rng.integers(1, 65))
                els.append(copy(off, n))
                produced += n
            elif kind == 4:
                # ts-page shape: off 8 / off 16 chains back to back
                els += [run(8, 640), run(16, 1280)] if produced >= 16 \
                    else [run(1, 64)]
                produced += 1920 if produced >= 16 else 64
            else:
                n = int(rng.integers(1, 7))
                els.append(lit(rnd(rng, n)))
                els.append(copy(int(rng.choice([1, 2, 4, 8]))
                                if produced + n >= 8 else 1,
                                int(rng.integers(4, 12))))
                produced = len(expand(b"".join(els)))
        cases.append((f"mixed#{i}", build(els)))
    check_exact(cases)


# ---------------------------------------------------------------------------
# store level: stored pages are read in place
# ---------------------------------------------------------------------------
def single_literal(comp, ulen):
    """This file's own tag walker: is the stream preamble + one literal
    covering everything?"""
    pos, v, sh = 0, 0, 0
    while True:
        b = comp[pos]
        pos += 1
        v |= (b & 0x7F) << sh
        if not b & 0x80:
            break
        sh += 7
    tag = comp[pos]
    if v != ulen or tag & 3:
        return False
    ln = (tag >> 2) + 1
    pos += 1
    if ln > 60:
        nb = ln - 60
        ln = int.from_bytes(comp[pos:pos + nb], "little") + 1
        pos += nb
    return ln == ulen and pos + ln == len(comp)


def count_stored_pages(series, ts, value, row_group=8192):
    """Per column, how many row-group pages pyarrow's snappy (the codec that
    writes the SSTs) emits as a single literal."""
    import pyarrow as pa
    codec = pa.Codec("snappy")
    counts = {"series": 0, "ts": 0, "value": 0, "pages": 0}
    for name, arr in (("series", np.asarray(series, np.uint64)),
                      ("ts", np.asarray(ts, np.int64)),
                      ("value", np.asarray(value, np.float64))):
        for s in range(0, len(arr), row_group):
            raw = arr[s:s + row_group].tobytes()
            counts["pages"] += 1
            if single_literal(codec.compress(raw, asbytes=True), len(raw)):
                counts[name] += 1
    return counts


def sst_paths(store_dir):
    ddir = os.path.join(store_dir, "data")
    return sorted((os.path.join(ddir, f) for f in os.listdir(ddir)
                   if f.endswith(".sst")),
                  key=lambda p: int(os.path.basename(p).split(".")[0]))


def check_agg(store_dir, ts_range, ssts):
    """scan_agg through a prepared scan vs the oracle; returns the scan's
    decode_stats()."""
    from horaedb_amd import Store
    with Store(store_dir) as st:
        with st.prepare(ts_range, devices=[0]) as pr:
            res = pr.exec_agg(ops=OPS)
            ds = pr.decode_stats()
    exp = oracle.scan_agg(ssts, ts_range, ops=OPS)
    assert res["series_id"].tolist() == exp["series_id"].tolist()
    assert res["count"].tolist() == exp["count"].tolist()
    np.testing.assert_array_equal(res["vmin"], exp["vmin"])
    np.testing.assert_array_equal(res["vmax"], exp["vmax"])
    np.testing.assert_allclose(res["sum"], exp["sum"], rtol=1e-9)
    return ds


def check_rows(store_dir, ts_range, ssts):
    from horaedb_amd import Store
    with Store(store_dir) as st:
        res = st.scan(ts_range, devices=[0])
    exp = oracle.scan_rows(ssts, ts_range, segment_ms=12 * 3600 * 1000)
    assert res["series_id"].tolist() == exp["series_id"].tolist()
    assert res["timestamp"].tolist() == exp["timestamp"].tolist()
    np.testing.assert_array_equal(res["value"], exp["value"])


def random_rows(rng, n, ts0):
    series = np.unique(rng.integers(0, 2**63, n, dtype=np.uint64))
    assert len(series) == n  # unique (a collision among 2^63 is a seed bug)
    ts = ts0 + np.cumsum(rng.integers(1, 1000, n)).astype(np.int64)
    value = rng.standard_normal(n)
    return series, ts, value


@pytest.fixture(scope="module")
def stored_store(tmp_path_factory):
    """Two time-disjoint Snappy SSTs: 2*8192+37 rows (64 KB pages and a
    296-byte tail page) and 5 rows (40-byte pages: inline literal length)."""
    rng = np.random.default_rng(11)
    out = str(tmp_path_factory.mktemp("stored"))
    a = random_rows(rng, 2 * 8192 + 37, 1_000_000)
    b = random_rows(rng, 5, int(a[1][-1]) + 10_000)
    want = {"series": 0, "ts": 0, "value": 0, "pages": 0}
    for seq, (s, t, v) in ((1, a), (2, b)):
        # rows are already (series, ts)-sorted: series unique ascending
        gen_sst_from_arrays(out, seq, s, t, v, sort=False,
                            compression="snappy")
        for k, c in count_stored_pages(s, t, v).items():
            want[k] += c
    ssts = [oracle.read_sst(p) for p in sst_paths(out)]
    return out, ssts, want, (int(a[1][0]), int(b[1][-1]) + 1)


def test_stored_pages_in_place_full_range(stored_store):
    out, ssts, want, (lo, hi) = stored_store
    # the walker must find stored pages in both the series and value columns
    assert want["series"] > 0 and want["value"] > 0
    ds = check_agg(out, (lo, hi), ssts)
    n_stored = want["series"] + want["ts"] + want["value"]
    assert ds["pages_in_place"] == n_stored
    assert ds["pages_decoded"] == want["pages"] - n_stored
    assert ds["bytes_in_place"] > 0
    assert (ds["bytes_in_place"] + ds["bytes_decoded_out"] ==
            8 * 3 * (2 * 8192 + 37 + 5))


def test_stored_pages_in_place_middle_range(stored_store):
    out, ssts, want, (lo, hi) = stored_store
    q = (hi - lo) // 4
    ds = check_agg(out, (lo + q, hi - q), ssts)
    assert ds["pages_in_place"] > 0


def test_stored_pages_scan_rows(stored_store):
    out, ssts, want, (lo, hi) = stored_store
    check_rows(out, (lo, hi), ssts)
    q = (hi - lo) // 4
    check_rows(out, (lo + q, hi - q), ssts)


def test_stored_pages_overlap_pair(tmp_path):
    # two generations of the same PKs: the dedup path's dense (series, ts)
    # copies read the stored pages from their shifted blob offsets
    rng = np.random.default_rng(12)
    out = str(tmp_path)
    s, t, v = random_rows(rng, 8192 + 37, 5_000)
    gen_sst_from_arrays(out, 1, s, t, v, sort=False, compression="snappy")
    keep = rng.random(len(s)) < 0.7
    gen_sst_from_arrays(out, 2, s[keep], t[keep],
                        rng.standard_normal(int(keep.sum())), sort=False,
                        compression="snappy")
    ssts = [oracle.read_sst(p) for p in sst_paths(out)]
    lo, hi = int(t[0]), int(t[-1]) + 1
    ds = check_agg(out, (lo, hi), ssts)
    assert ds["pages_in_place"] > 0
    check_agg(out, (lo + (hi - lo) // 4, hi - (hi - lo) // 4), ssts)
    check_rows(out, (lo, hi), ssts)


def test_bench_shaped_mini_dataset(tmp_path):
    # 64 windows over 100 points: files with 1 and with 2 points per series
    out = str(tmp_path)
    m = gen_dataset(out, n_rows=200_000, n_series=2_000, n_ssts=64,
                    compression="snappy")
    assert {s["rows"] for s in m["ssts"]} == {2_000, 4_000}
    lo, hi = middle_range(m)
    in_range = [s for s in m["ssts"]
                if s["ts_min"] < hi and s["ts_max"] >= lo]
    ssts = [oracle.read_sst(s["path"]) for s in m["ssts"]]
    ds = check_agg(out, (lo, hi), ssts)
    total_pages = 3 * len(in_range)   # one row group per file
    assert ds["pages_in_place"] + ds["pages_decoded"] == total_pages
    assert ds["pages_in_place"] > 0
    assert ds["pages_decoded"] < total_pages
