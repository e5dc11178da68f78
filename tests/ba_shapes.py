# Shapes for kernel 1f (PLAIN BYTE_ARRAY page images from value handles) and
# its host twin, shared by test_bytes_write_cpu.py and test_bytes_write_gpu.py.
# Everything is built from fixed seeds. The expectation is the definition of
# the page: per output row struct.pack("<I", len) + value, joined.
import struct

import numpy as np

LENS = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 4097]
MAX_LEN = (1 << 20) - 1
ROW_GROUP = 8192


def make_source(lens, seed, aligns=None):
    """Source bytes holding one value per length, value i at an offset whose
    residue modulo 16 is aligns[i] (default: i % 16), with random filler
    between. Returns (src bytes, handles uint64[len(lens)])."""
    rng = np.random.default_rng(seed)
    n = len(lens)
    offs = np.zeros(n, dtype=np.int64)
    pos = 0
    for i, ln in enumerate(lens):
        want = (i % 16) if aligns is None else aligns[i]
        pos += (want - pos) % 16
        offs[i] = pos
        pos += ln
    src = rng.integers(0, 256, max(pos, 1), dtype=np.uint8).tobytes()[:pos]
    handles = (offs.astype(np.uint64) << np.uint64(20)) | \
        np.asarray(lens, dtype=np.uint64)
    return src, handles


def expected_pages(src, handles, group_start=None, n_out=None,
                   row_group=ROW_GROUP, refused=()):
    """The page images by definition; rows in `refused` are empty values."""
    n_src = len(handles)
    if n_out is None:
        n_out = n_src if group_start is None else len(group_start) - 1
    offs = (np.asarray(handles, dtype=np.uint64) >> np.uint64(20)).tolist()
    lens = (np.asarray(handles, dtype=np.uint64) &
            np.uint64(0xFFFFF)).tolist()
    pages = []
    for r0 in range(0, n_out, row_group):
        parts = []
        for i in range(r0, min(n_out, r0 + row_group)):
            if i in refused:
                parts.append(struct.pack("<I", 0))
                continue
            a, b = (i, i + 1) if group_start is None else \
                (int(group_start[i]), int(group_start[i + 1]))
            v = b"".join(src[offs[j]:offs[j] + lens[j]] for j in range(a, b))
            parts.append(struct.pack("<I", len(v)) + v)
        pages.append(b"".join(parts))
    return pages


def lens_by_alignment():
    """Every length of LENS and one of 2^20 - 1 at each source offset
    0..15 mod 16, mixed in one page."""
    rng = np.random.default_rng(41)
    lens, aligns = [], []
    for ln in LENS:
        for a in range(16):
            lens.append(ln)
            aligns.append(a)
    order = rng.permutation(len(lens))
    lens = [lens[i] for i in order]
    aligns = [aligns[i] for i in order]
    lens.insert(100, MAX_LEN)
    aligns.insert(100, 5)
    return make_source(lens, 42, aligns)


ROW_COUNTS = [1, 63, 64, 65, 8191, 8192, 8193, 20000]


def rows_case(n):
    """n rows (20 000: three row groups, the last short), short lengths so
    the volume stays small, every alignment."""
    rng = np.random.default_rng(1000 + n)
    lens = rng.choice(LENS[:12], size=n).tolist()
    aligns = rng.integers(0, 16, n).tolist()
    return make_source(lens, 2000 + n, aligns)


def groups_case():
    """Group sizes 1, 2, 63, 64, 65, 300, a group of nothing but empty
    values, a group straddling source row 8192 (a row-group edge of the
    SOURCE rows) and one whose total is exactly 2^20 - 1. 8 190 single-row
    groups in front make it two output row groups."""
    rng = np.random.default_rng(77)
    sizes = [1] * 8190 + [6, 1, 2, 63, 64, 65, 300, 40, 3, 1]
    gs = np.concatenate(([0], np.cumsum(sizes))).astype(np.uint32)
    n_src = int(gs[-1])
    lens = rng.choice(LENS[:11], size=n_src).tolist()
    g_empty = len(sizes) - 3
    for j in range(int(gs[g_empty]), int(gs[g_empty + 1])):
        lens[j] = 0
    g_cap = len(sizes) - 2          # three rows: 2^19 + (2^19 - 18) + 17
    a = int(gs[g_cap])
    lens[a], lens[a + 1], lens[a + 2] = 1 << 19, (1 << 19) - 18, 17
    aligns = rng.integers(0, 16, n_src).tolist()
    src, handles = make_source(lens, 78, aligns)
    return src, handles, gs
