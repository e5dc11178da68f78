# Staging of one column chunk (horaedb_amd/csrc/stage_chunk.{h,cpp}), host
# side, no GPU: `make stage_check` builds a stand-alone program (ASan+UBSan
# when the host compiler links them) that stages every chunk of the SSTs
# written here into a heap block of exactly the reserved size, checks its own
# bounds assertions, mutates some of the chunks (seeded), and prints one
# record per chunk. The records are compared here with what pyarrow reads
# from the same files.
import json
import os
import subprocess

import numpy as np
import pytest

from test_optional_cpu import _zstd_loadable, write_nullable_sst
from tools.gen_ssts import write_bytes_sst, write_sst

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "horaedb_amd", "csrc")

ROWS = [1, 63, 64, 100, 8191, 8192, 8193]
CODECS = ["none", "snappy"] + (["zstd"] if _zstd_loadable() else [])
STAGED = ("series_id", "timestamp", "value", "__seq__")


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    series = np.sort(rng.integers(0, 1 << 62, n, dtype=np.uint64))
    ts = np.arange(n, dtype=np.int64) * 1000
    return rng, series, ts


def _write_all(d):
    """name -> argument prefix for the check program ('' / 'fuzz:' / 'tight:')"""
    files = {}
    for codec in CODECS:
        for ver in ("1.0", "2.0"):
            for n in ROWS:
                rng, series, ts = _rows(n, n)
                v = ver[0]
                write_sst(f"{d}/req_{codec}_v{v}_{n}.sst", series, ts,
                          rng.random(n), 1, compression=codec,
                          data_page_version=ver)
                files[f"req_{codec}_v{v}_{n}.sst"] = ""
                for tag, frac in (("opt", 0.0), ("nul", 0.3)):
                    name = f"{tag}_{codec}_v{v}_{n}.sst"
                    write_nullable_sst(f"{d}/{name}", series, ts,
                                       rng.random(n), 1,
                                       value_null=rng.random(n) < frac,
                                       compression=codec, version=ver)
                    files[name] = ""
        for n in (100, 8192):
            rng, series, ts = _rows(n, n + 1)
            write_sst(f"{d}/delta_{codec}_{n}.sst", series, ts, rng.random(n),
                      1, compression=codec,
                      ts_encoding="DELTA_BINARY_PACKED")
            files[f"delta_{codec}_{n}.sst"] = ""
            # two rows per series: a dictionary half the column's size
            dser = np.repeat(np.arange(n // 2, dtype=np.uint64) << 32, 2)
            write_sst(f"{d}/dict_{codec}_{n}.sst", dser, ts, rng.random(n), 1,
                      compression=codec, dict_columns=("series_id",))
            files[f"dict_{codec}_{n}.sst"] = ""
            # compressible values take the Snappy decoder, random ones are
            # stored literals read in place
            write_sst(f"{d}/flat_{codec}_{n}.sst", series, ts,
                      np.full(n, 2.5), 1, compression=codec)
            files[f"flat_{codec}_{n}.sst"] = ""
            write_sst(f"{d}/rand_{codec}_{n}.sst", series, ts, rng.random(n),
                      1, compression=codec)
            files[f"rand_{codec}_{n}.sst"] = ""
    for n in (100, 8192):
        rng, series, ts = _rows(n, n + 2)
        write_bytes_sst(f"{d}/bytes_{n}.sst", series, ts,
                        [b"v%d" % i * (1 + i % 3) for i in range(n)], 1)
        files[f"bytes_{n}.sst"] = ""
    for name in ("nul_snappy_v1_100.sst", "nul_snappy_v2_8192.sst",
                 "req_none_v1_100.sst", "opt_none_v1_100.sst",
                 "dict_snappy_100.sst", "delta_snappy_100.sst",
                 "nul_zstd_v1_100.sst", "nul_zstd_v2_100.sst",
                 "dict_zstd_100.sst"):
        if name in files:
            files[name] = "fuzz:"
    for name in ("flat_zstd_8192.sst", "dict_zstd_8192.sst"):
        if name in files:
            files[name] = "tight:"
    return files


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("stage"))
    files = _write_all(d)
    b = subprocess.run(["make", "-C", CSRC, "stage_check"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(CSRC, "stage_check")] +
                       [f"{pre}{d}/{name}" for name, pre in files.items()],
                       capture_output=True, text=True)
    lines = r.stdout.strip().splitlines()
    recs = [json.loads(ln[4:]) for ln in lines if ln.startswith("REC ")]
    print(b.stdout + "\n".join(ln for ln in lines
                               if not ln.startswith(("REC ", "  "))))
    return {"dir": d, "files": files, "proc": r, "lines": lines, "recs": recs}


def test_stage_check_program(run):
    r, lines = run["proc"], run["lines"]
    assert r.returncode == 0, "\n".join(lines[-20:]) + r.stderr[-4000:]
    assert lines[-1] == "ALL OK"
    assert not any(ln.endswith("FAIL") for ln in lines)
    assert any(ln.startswith("slice_and_order over") for ln in lines)
    hostile = [ln for ln in lines if ln.startswith("hostile ") and
               "mutations" in ln]
    assert len(hostile) == sum(p == "fuzz:" for p in run["files"].values())
    for ln in hostile:
        w = ln.replace(",", "").split()
        n, staged, refused = int(w[2]), int(w[4]), int(w[6])
        assert n >= 2000 and staged + refused == n and refused > 0
    if "zstd" in CODECS:
        tight = [ln for ln in lines if ln.startswith("tight ") and
                 ln.endswith("refused OK")]
        assert any("data page" in ln for ln in tight)
        assert any("dictionary page" in ln for ln in tight)


def _expected(run):
    """(file, rg, col) -> pyarrow column of that row group"""
    import pyarrow.parquet as pq
    out = {}
    for name in run["files"]:
        pf = pq.ParquetFile(os.path.join(run["dir"], name))
        for rg in range(pf.num_row_groups):
            tbl = pf.read_row_group(rg)
            for col in STAGED:
                out[name, rg, col] = tbl[col].combine_chunks()
    return out


def test_records_match_pyarrow(run):
    exp = _expected(run)
    recs = {(r["file"], r["rg"], r["col"]): r for r in run["recs"]}
    assert set(recs) == set(exp)   # every chunk staged, once
    n_body = n_packed = n_bitmap = 0
    for key, col in exp.items():
        r = recs[key]
        valid = col.is_valid().to_numpy(zero_copy_only=False)
        assert r["n_valid"] == int(valid.sum()), key
        assert r["has_nulls"] == int(not valid.all()), key
        if r["bitmap"]:
            bits = np.unpackbits(np.frombuffer(bytes.fromhex(r["bitmap"]),
                                               dtype=np.uint8),
                                 bitorder="little")
            np.testing.assert_array_equal(bits[:len(valid)], valid, str(key))
            assert not bits[len(valid):].any(), key
            n_bitmap += 1
        if key[0].startswith("bytes_") and key[2] == "value":
            assert r["ba"] == 1
            continue
        want = col.drop_null().to_numpy(zero_copy_only=False).tobytes()
        if r["where"] == "blob":
            assert r["off_mod64"] == 0, key
            assert bytes.fromhex(r["body"]) == want, key
            n_body += 1
        if r["packed"]:
            assert bytes.fromhex(r["packed"]) == want, key
            n_packed += 1
    # validity words exist for the value chunk of every OPTIONAL file
    assert n_bitmap == sum(k[0].startswith(("opt_", "nul_")) and
                           k[2] == "value" for k in exp)
    assert n_body > 0 and n_packed > 0


def test_snappy_pages_accounted(run):
    # files without OPTIONAL columns: every Snappy page written is either
    # read in place or handed to the decoder, dictionary pages included
    import pyarrow.parquet as pq
    recs = {(r["file"], r["rg"], r["col"]): r for r in run["recs"]}
    stored = decoded = 0
    for name in run["files"]:
        if "_snappy_" not in name or name.startswith(("opt_", "nul_")):
            continue
        md = pq.ParquetFile(os.path.join(run["dir"], name)).metadata
        for g in range(md.num_row_groups):
            for c in STAGED:
                cm = md.row_group(g).column(md.schema.names.index(c))
                r = recs[name, g, c]
                mine = r["in_place"] + r["snappy"]
                # a v2 page that compression would not shrink is written
                # uncompressed (is_compressed = false): not a Snappy page
                if "_v2_" in name and mine == 0:
                    assert cm.total_compressed_size == \
                        cm.total_uncompressed_size, (name, g, c)
                    continue
                assert mine == 1 + cm.has_dictionary_page, (name, g, c)
                stored += r["in_place"]
                decoded += r["snappy"]
    assert stored > 0 and decoded > 0   # both routes occurred
