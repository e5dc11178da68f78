# Value shapes for kernel 1g (k_ba_page_minmax) and its host twin: each case
# is (name, values, row_group, skip). The expectation is Python's own
# min()/max() over bytes (lexicographic on unsigned bytes, a proper prefix is
# smaller), with the writer's rule on top: no statistics when either bound is
# longer than 64 bytes. Shared by the CPU and the GPU tests.
import numpy as np

ROW_COUNTS = [1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193]
MAX_LEN = (1 << 20) - 1


def _rand_values(rng, n, max_len=20):
    lens = rng.integers(0, max_len + 1, n)
    blob = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8).tobytes()
    ends = np.cumsum(lens)
    return [blob[e - k:e] for e, k in zip(ends.tolist(), lens.tolist())]


def expected(values, row_group=8192, skip=()):
    vals = [b"" if i in set(skip) else bytes(v) for i, v in enumerate(values)]
    out = []
    for g in range(0, len(vals), row_group):
        page = vals[g:g + row_group]
        mn, mx = min(page), max(page)
        out.append((mn, mx) if len(mn) <= 64 and len(mx) <= 64 else None)
    return out


def cases():
    rng = np.random.default_rng(41)
    out = []
    for n in ROW_COUNTS:
        out.append((f"rows{n}", _rand_values(rng, n), 8192, ()))
    # small row groups: several pages, the last short
    out.append(("pages_of_100", _rand_values(rng, 1000), 100, ()))
    out.append(("all_equal", [b"same value"] * 300, 8192, ()))
    out.append(("all_empty", [b""] * 70, 8192, ()))
    vals = _rand_values(rng, 500, 12)
    vals = [v or b"x" for v in vals]
    vals[123] = b""
    out.append(("empty_is_min", vals, 8192, ()))
    out.append(("high_bytes", [b"\x7f\xff", b"\x80", b"\xff\x00", b"\x00\xff",
                               b"\xfe\xff\xff"] * 30, 8192, ()))
    # the min or the max at the first, an inner and the last row
    for where, i in (("first", 0), ("inner", 300), ("last", 599)):
        for kind, v in (("min", b"\x01"), ("max", b"\xfe" * 9)):
            vals = [b"\x40" + v2 for v2 in _rand_values(rng, 600, 10)]
            vals[i] = v
            out.append((f"{kind}_{where}", vals, 8192, ()))
    # values sharing a long prefix and differing only behind it
    for p in (63, 64, 65, 66):
        pre = bytes(rng.integers(0, 256, p, dtype=np.uint8).tolist())
        vals = [pre + bytes([b]) + b"tail" for b in (7, 3, 200, 3, 9)] * 20
        out.append((f"prefix{p}", vals, 8192, ()))
        # the bounds themselves short, the long ones in between
        out.append((f"prefix{p}_inside",
                    [b"\x00"] + vals + [b"\xff\xff"], 8192, ()))
    out.append(("min_64_kept", [b"a" * 64, b"b", b"a" * 64 + b"z"], 8192, ()))
    out.append(("min_65_omitted", [b"a" * 65, b"b", b"a" * 65 + b"z"], 8192,
                ()))
    out.append(("max_64_kept", [b"z" * 64, b"b", b"z" * 63], 8192, ()))
    out.append(("short_min_long_max", [b"b", b"zz" * 35, b"c"], 8192, ()))
    out.append(("long_min_short_max", [b"\x00" * 70, b"b", b"c"], 8192, ()))
    # a 65-byte key that equals the first 65 bytes of a longer value
    out.append(("key_ties", [b"m" * 65, b"m" * 66, b"m" * 64, b"m" * 200],
                8192, ()))
    big = bytes(rng.integers(1, 255, MAX_LEN, dtype=np.uint8).tolist())
    out.append(("one_value_at_the_limit", [b"k", big, b"\x00q"], 8192, ()))
    vals = _rand_values(rng, 200, 30)
    vals = [v or b"y" for v in vals]
    out.append(("refused_row", vals, 8192, (17,)))
    # every start alignment modulo 8: row sizes 4 + len walk all residues,
    # and the compare has to go past the first words
    pre = b"0123456789abcdefghijklmnopqrs"
    vals = [pre[:8 + (i * 5) % 21] + bytes([i % 251]) * (i % 8)
            for i in range(400)]
    out.append(("every_alignment", vals, 8192, ()))
    vals = [bytes([65 + (i * 7) % 26]) * (i % 9) for i in range(2000)]
    out.append(("short_values_every_alignment", vals, 512, ()))
    return out
