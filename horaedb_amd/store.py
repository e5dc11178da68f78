# horaedb_amd/store.py — ctypes binding of the C-ABI (include/horaedb_hx.h).
# Store mirrors the reference's ColumnarStorage trait surface
# (storage.rs:76-89): schema contract fixed by the metric engine, scan via
# scan_agg (hot path) and scan (streaming parity mode).
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libhoraedb_hx.so")

AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX, AGG_AVG = 1, 2, 4, 8, 16
AGG_FIRST, AGG_LAST = 32, 64

_ERRNAMES = {0: "OK", 1: "IO", 2: "FORMAT", 3: "UNSUPPORTED", 4: "NO_GPU",
             5: "HIP", 6: "INVALID", 7: "SCHEMA"}


class HxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"hx error {_ERRNAMES.get(code, code)}: {msg}")
        self.code = code


class _TimeRange(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64)]


class _SstDesc(C.Structure):
    _fields_ = [("path", C.c_char_p), ("sequence", C.c_uint64)]


class _Pred(C.Structure):
    _fields_ = [("kind", C.c_int32), ("series_ids", C.POINTER(C.c_uint64)),
                ("n_series", C.c_size_t)]


class _ScanSpec(C.Structure):
    _fields_ = [("range", _TimeRange), ("preds", C.POINTER(_Pred)),
                ("n_preds", C.c_size_t), ("ssts", C.POINTER(_SstDesc)),
                ("n_ssts", C.c_size_t), ("projection", C.POINTER(C.c_int32)),
                ("n_projection", C.c_size_t)]


class _AggSpec(C.Structure):
    _fields_ = [("ops", C.c_uint32), ("bucket_ms", C.c_int64)]


class _DeviceSet(C.Structure):
    _fields_ = [("device_ids", C.POINTER(C.c_int32)), ("n_devices", C.c_int32)]


class _ResultTable(C.Structure):
    _fields_ = [("n_groups", C.c_size_t),
                ("series_id", C.POINTER(C.c_uint64)),
                ("bucket", C.POINTER(C.c_int64)),
                ("sum", C.POINTER(C.c_double)),
                ("count", C.POINTER(C.c_uint64)),
                ("vmin", C.POINTER(C.c_double)),
                ("vmax", C.POINTER(C.c_double)),
                ("avg", C.POINTER(C.c_double)),
                ("first", C.POINTER(C.c_double)),
                ("first_ts", C.POINTER(C.c_int64)),
                ("last", C.POINTER(C.c_double)),
                ("last_ts", C.POINTER(C.c_int64))]


class _ColBatch(C.Structure):
    _fields_ = [("n_rows", C.c_size_t), ("n_cols", C.c_size_t),
                ("cols", C.POINTER(C.c_void_p)),
                ("col_types", C.POINTER(C.c_int32)),
                ("validity", C.POINTER(C.POINTER(C.c_uint8)))]


class _ExecStats(C.Structure):
    _fields_ = [("exec_ms", C.c_double), ("agg_kernel_ms", C.c_double),
                ("decode_kernel_ms", C.c_double), ("rows_scanned", C.c_int64),
                ("rows_matched", C.c_int64), ("bytes_staged", C.c_int64),
                ("stage_ms", C.c_double)]


class _DecodeStats(C.Structure):
    _fields_ = [("pages_in_place", C.c_uint64), ("pages_decoded", C.c_uint64),
                ("bytes_in_place", C.c_uint64),
                ("bytes_decoded_out", C.c_uint64)]


def _load():
    if not os.path.exists(_LIB):
        raise ImportError(
            f"{_LIB} missing — build it with `make -C horaedb_amd/csrc` "
            "(the HIP product path; no CPU fallback exists)")
    lib = C.CDLL(_LIB)
    lib.hx_last_error.restype = C.c_char_p
    lib.hx_open.argtypes = [C.c_char_p, C.c_int64, C.POINTER(C.c_void_p)]
    lib.hx_close.argtypes = [C.c_void_p]
    lib.hx_find_ssts.argtypes = [C.c_void_p, _TimeRange,
                                 C.POINTER(C.POINTER(_SstDesc)),
                                 C.POINTER(C.c_size_t)]
    lib.hx_prepare.argtypes = [C.c_void_p, C.POINTER(_ScanSpec),
                               C.POINTER(_DeviceSet), C.POINTER(C.c_void_p)]
    lib.hx_prepared_free.argtypes = [C.c_void_p]
    lib.hx_exec_agg.argtypes = [C.c_void_p, C.POINTER(_AggSpec),
                                C.POINTER(C.POINTER(_ResultTable))]
    lib.hx_result_free.argtypes = [C.POINTER(_ResultTable)]
    lib.hx_scan_agg.argtypes = [C.c_void_p, C.POINTER(_ScanSpec),
                                C.POINTER(_AggSpec), C.POINTER(_DeviceSet),
                                C.POINTER(C.POINTER(_ResultTable))]
    lib.hx_get_stats.argtypes = [C.c_void_p, C.POINTER(_ExecStats)]
    lib.hx_get_decode_stats.argtypes = [C.c_void_p, C.POINTER(_DecodeStats)]
    lib.hx_scan.argtypes = [C.c_void_p, C.POINTER(_ScanSpec),
                            C.POINTER(_DeviceSet), C.c_void_p, C.c_void_p]
    lib.hx_compact.argtypes = [C.c_void_p, _TimeRange, C.POINTER(_DeviceSet),
                               C.POINTER(C.c_uint64)]
    lib.hx_write.argtypes = [C.c_void_p, C.POINTER(C.c_uint64),
                             C.POINTER(C.c_int64), C.POINTER(C.c_double),
                             C.c_int64, C.c_int32, C.POINTER(C.c_uint64)]
    lib.hx_write_sst.argtypes = [C.c_char_p, C.POINTER(C.c_uint64),
                                 C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                 C.c_uint64, C.c_int64, C.c_int64]
    lib.hx_set_nullable_values.argtypes = [C.c_void_p, C.c_int32]
    lib.hx_write_nullable.argtypes = [
        C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int64),
        C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_int64, C.c_int32,
        C.POINTER(C.c_uint64)]
    lib.hx_write_sst_nullable.argtypes = [
        C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int64),
        C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_uint64, C.c_int64,
        C.c_int64]
    lib.hx_set_write_codec.argtypes = [C.c_void_p, C.c_int32]
    lib.hx_write_sst_codec.argtypes = [
        C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int64),
        C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_int32, C.c_uint64,
        C.c_int64, C.c_int64, C.c_int32]
    lib.hx_debug_snappy_compress_host.argtypes = [
        C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.hx_debug_snappy_compress_host.restype = C.c_uint64
    lib.hx_debug_snappy_compress.argtypes = [
        C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_uint32,
        C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint64),
        C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.hx_debug_pack_optional.argtypes = [
        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8),
        C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32,
        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
        C.POINTER(C.c_uint64)]
    lib.hx_write_bytes.argtypes = [
        C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.c_void_p,
        C.POINTER(C.c_int64), C.c_int64, C.c_int32, C.POINTER(C.c_uint64)]
    lib.hx_write_sst_bytes.argtypes = [
        C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.c_void_p,
        C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.c_uint64, C.c_int64,
        C.c_int64]
    lib.hx_write_sst_bytes_codec.argtypes = \
        lib.hx_write_sst_bytes.argtypes + [C.c_int32]
    lib.hx_set_bytes_write_codec.argtypes = [C.c_void_p, C.c_int32]
    lib.hx_write_sst_bytes_paged.argtypes = \
        lib.hx_write_sst_bytes_codec.argtypes + [C.c_uint32]
    lib.hx_set_bytes_page_limit.argtypes = [C.c_void_p, C.c_uint32]
    for f in (lib.hx_debug_ba_batch_sizes, lib.hx_debug_ba_batch_sizes_host):
        f.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
                      C.POINTER(C.c_uint64)]
    for f in (lib.hx_debug_ba_page_minmax, lib.hx_debug_ba_page_minmax_host):
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64),
                      C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
                      C.c_void_p]
    for f in (lib.hx_debug_ba_pages, lib.hx_debug_ba_pages_host):
        f.argtypes = [
            C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32,
            C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
            C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64,
            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.hx_schema.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t),
                              C.POINTER(C.c_size_t)]
    lib.hx_catalog_size.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    lib.hx_catalog_entry.argtypes = [C.c_void_p, C.c_size_t,
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64)]
    lib.hx_debug_page_levels.argtypes = [
        C.c_char_p, C.c_int32, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint64,
        C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    return lib


_lib = _load()


def lib_path():
    return _LIB


def _check(code):
    if code != 0:
        raise HxError(code, _lib.hx_last_error().decode())


def _np(ptr, n, dtype):
    if not ptr or n == 0:
        return np.empty(0, dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


class HeldResult:
    """An exec_agg result still held in the library's host buffer (the
    hx_result_table the C caller receives). take() copies rows out as numpy
    arrays; close() hands the buffer back (hx_result_free)."""

    def __init__(self, out, ops, bucket_ms):
        self._out = out
        self._ops = ops
        self._bucket_ms = bucket_ms
        self.n_groups = out.contents.n_groups

    def take(self, idx=None):
        """The result columns as numpy copies: every group (idx=None) or
        the rows of the index array idx."""
        t = self._out.contents
        n = self.n_groups
        ops = self._ops

        def col(ptr, dtype):
            if idx is None or not ptr or n == 0:
                return _np(ptr, n, dtype)
            return np.ctypeslib.as_array(ptr, shape=(n,))[idx].astype(
                dtype, copy=False)

        res = {"series_id": col(t.series_id, np.uint64)}
        if self._bucket_ms:
            res["bucket"] = col(t.bucket, np.int64)
        if ops & AGG_SUM:
            res["sum"] = col(t.sum, np.float64)
        if ops & AGG_COUNT:
            res["count"] = col(t.count, np.uint64)
        if ops & AGG_MIN:
            res["vmin"] = col(t.vmin, np.float64)
        if ops & AGG_MAX:
            res["vmax"] = col(t.vmax, np.float64)
        if ops & AGG_AVG:
            res["avg"] = col(t.avg, np.float64)

        def bits_col(ptr):
            # the value columns of first/last travel as 64-bit words, so the
            # float64 arrays carry the stored bits (NaN payloads included)
            return col(C.cast(ptr, C.POINTER(C.c_uint64)),
                       np.uint64).view(np.float64)

        if ops & AGG_FIRST:
            res["first"] = bits_col(t.first)
            res["first_ts"] = col(t.first_ts, np.int64)
        if ops & AGG_LAST:
            res["last"] = bits_col(t.last)
            res["last_ts"] = col(t.last_ts, np.int64)
        return res

    def close(self):
        if self._out is not None:
            _lib.hx_result_free(self._out)
            self._out = None


class Prepared:
    """A staged scan (column chunks resident in HBM). exec_agg is the timed
    hot path."""

    def __init__(self, store, handle):
        self._store = store
        self._h = handle

    def exec_agg(self, ops=AGG_SUM | AGG_COUNT, bucket_ms=0, copy=True,
                 hold=False):
        """copy=False: run the full query (result lands in host memory) but
        skip the numpy materialization — for benchmarking loops.
        hold=True: same run, but return the result still in the library's
        buffer as a HeldResult (the caller copies out later and closes it)."""
        spec = _AggSpec(ops=ops, bucket_ms=bucket_ms)
        out = C.POINTER(_ResultTable)()
        _check(_lib.hx_exec_agg(self._h, C.byref(spec), C.byref(out)))
        held = HeldResult(out, ops, bucket_ms)
        if hold:
            return held
        try:
            return held.take() if copy else {"n_groups": held.n_groups}
        finally:
            held.close()

    def stats(self):
        st = _ExecStats()
        _check(_lib.hx_get_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def decode_stats(self):
        """What staging did with the Snappy pages: stored (single-literal)
        pages read in place vs pages the GPU decoder expands."""
        st = _DecodeStats()
        _check(_lib.hx_get_decode_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def close(self):
        if self._h:
            _lib.hx_prepared_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class _TagPred(C.Structure):
    _fields_ = [("tag_key", C.c_char_p), ("tag_value", C.c_char_p)]


class _BytesCol(C.Structure):
    _fields_ = [("offsets", C.POINTER(C.c_int64)),
                ("bytes", C.POINTER(C.c_uint8))]


class Store:
    """MI355X-native ColumnarStorage (scan side). storage.rs:76-89."""

    def __init__(self, store_path, segment_duration_ms=0,
                 update_mode="overwrite"):
        h = C.c_void_p()
        self._update_mode = update_mode
        _check(_lib.hx_open(store_path.encode(), segment_duration_ms,
                            C.byref(h)))
        self._h = h
        if update_mode == "append":
            _check(_lib.hx_set_update_mode(self._h, 1))
        elif update_mode != "overwrite":
            raise ValueError("update_mode: 'overwrite' or 'append'")

    def close(self):
        if self._h:
            _lib.hx_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def schema(self):
        """ColumnarStorage::schema (storage.rs:76-89): column layout with
        PK/builtin markers (types.rs:150-240 contract)."""

        class _Col(C.Structure):
            _fields_ = [("name", C.c_char_p), ("col_type", C.c_int32),
                        ("is_primary_key", C.c_int32),
                        ("is_builtin", C.c_int32)]

        out = C.POINTER(_Col)()
        n = C.c_size_t()
        npk = C.c_size_t()
        _check(_lib.hx_schema(self._h, C.cast(C.byref(out), C.c_void_p),
                              C.byref(n), C.byref(npk)))
        tnames = {0: "u64", 1: "i64", 2: "f64", 3: "binary"}
        cols = [{"name": out[i].name.decode(),
                 "type": tnames[out[i].col_type],
                 "primary_key": bool(out[i].is_primary_key),
                 "builtin": bool(out[i].is_builtin)} for i in range(n.value)]
        return {"columns": cols, "num_primary_keys": npk.value}

    def catalog(self):
        n = C.c_size_t()
        _check(_lib.hx_catalog_size(self._h, C.byref(n)))
        out = []
        for i in range(n.value):
            seq = C.c_uint64()
            rows = C.c_int64()
            tmin = C.c_int64()
            tmax = C.c_int64()
            nrg = C.c_int64()
            _check(_lib.hx_catalog_entry(self._h, i, C.byref(seq), C.byref(rows),
                                         C.byref(tmin), C.byref(tmax),
                                         C.byref(nrg)))
            out.append({"seq": seq.value, "n_rows": rows.value,
                        "ts_min": tmin.value, "ts_max": tmax.value,
                        "n_row_groups": nrg.value})
        return out

    def find_ssts(self, ts_range):
        """Manifest::find_ssts (manifest/mod.rs:165-172)."""
        out = C.POINTER(_SstDesc)()
        n = C.c_size_t()
        _check(_lib.hx_find_ssts(self._h, _TimeRange(*ts_range), C.byref(out),
                                 C.byref(n)))
        return [(out[i].path.decode(), out[i].sequence) for i in range(n.value)]

    def _spec(self, ts_range, series_in=None):
        # keepalive is CALL-LOCAL (returned, held by the caller until the C
        # call returns): a Store serves prepares from many threads
        spec = _ScanSpec()
        spec.range = _TimeRange(*ts_range)
        keep = []
        if series_in is not None:
            arr = np.ascontiguousarray(np.asarray(sorted(set(int(s) for s in series_in)),
                                                  dtype=np.uint64))
            pred = _Pred(kind=1,
                         series_ids=arr.ctypes.data_as(C.POINTER(C.c_uint64)),
                         n_series=len(arr))
            preds = (_Pred * 1)(pred)
            spec.preds = preds
            spec.n_preds = 1
            keep += [arr, preds]
        return spec, keep

    def _devset(self, devices, keep):
        if devices is None:
            return None
        ids = (C.c_int32 * len(devices))(*devices)
        ds = _DeviceSet(device_ids=ids, n_devices=len(devices))
        keep += [ids, ds]
        return ds

    def prepare(self, ts_range, series_in=None, devices=None,
                sst_subset=None):
        """sst_subset: list of (path, seq) to scan (hx_scan_spec.ssts — the
        per-GPU shard of BASELINE configs 4/5); None = all overlapping."""
        spec, keep = self._spec(ts_range, series_in)
        if sst_subset is not None:
            arr = (_SstDesc * len(sst_subset))()
            enc = [p.encode() for p, _ in sst_subset]
            for i, ((p, q), pe) in enumerate(zip(sst_subset, enc)):
                arr[i].path = pe
                arr[i].sequence = q
            spec.ssts = arr
            spec.n_ssts = len(sst_subset)
            keep += [arr, enc]
        ds = self._devset(devices, keep)
        out = C.c_void_p()
        _check(_lib.hx_prepare(self._h, C.byref(spec),
                               C.byref(ds) if ds else None, C.byref(out)))
        del keep
        return Prepared(self, out)

    def scan_agg(self, ts_range, ops=AGG_SUM | AGG_COUNT, bucket_ms=0,
                 series_in=None, devices=None):
        """One-shot scan+aggregate (prepare + exec + release)."""
        with self.prepare(ts_range, series_in, devices) as p:
            return p.exec_agg(ops=ops, bucket_ms=bucket_ms)

    def index_write(self, tag_keys, tag_values, tsids, metric_id=None):
        """Append one inverted-index SST (rfc:86-137 index table): rows
        (metric_id, tag_key, tag_value, tsid), writer-sorted by
        (tag_key, tag_value, tsid). Returns the index file sequence."""
        n = len(tsids)
        assert len(tag_keys) == n and len(tag_values) == n
        tk = (C.c_char_p * n)(*[k.encode() if isinstance(k, str) else k
                                for k in tag_keys])
        tv = (C.c_char_p * n)(*[v.encode() if isinstance(v, str) else v
                                for v in tag_values])
        tsids = np.ascontiguousarray(tsids, dtype=np.uint64)
        mid = None
        midp = None
        if metric_id is not None:
            mid = np.ascontiguousarray(metric_id, dtype=np.uint64)
            midp = mid.ctypes.data_as(C.POINTER(C.c_uint64))
        seq = C.c_uint64()
        _check(_lib.hx_index_write(
            self._h, midp, tk, tv,
            tsids.ctypes.data_as(C.POINTER(C.c_uint64)), n, C.byref(seq)))
        return int(seq.value)

    def index_query(self, preds, combine="and", device=0):
        """Tag-equality predicates -> sorted distinct TSID set (GPU
        postings filter + set combine). preds: [(key, value), ...]."""
        n = len(preds)
        arr = (_TagPred * n)()
        keep = []
        for i, (k, v) in enumerate(preds):
            kb = k.encode() if isinstance(k, str) else k
            vb = v.encode() if isinstance(v, str) else v
            keep += [kb, vb]
            arr[i].tag_key = kb
            arr[i].tag_value = vb
        out = C.POINTER(C.c_uint64)()
        n_out = C.c_size_t()
        _check(_lib.hx_index_query(self._h, arr, n,
                                   1 if combine == "and" else 0, device,
                                   C.byref(out), C.byref(n_out)))
        try:
            res = np.array(_np(out, n_out.value, np.uint64), copy=True) \
                if n_out.value else np.empty(0, np.uint64)
        finally:
            _lib.hx_tsids_free(out)
        return res

    def set_nullable_values(self, on):
        """Writer setting (hx_set_nullable_values): True makes every SST this
        store writes declare `value` OPTIONAL and keeps null values through
        write(valid=...), compact and compact_files."""
        _check(_lib.hx_set_nullable_values(self._h, 1 if on else 0))

    def set_write_codec(self, codec):
        """Writer setting (hx_set_write_codec): CODEC_NONE (default) or
        CODEC_SNAPPY, the page codec of every SST this store writes from now
        on (write, compact, compact_files); combines with
        set_nullable_values."""
        _check(_lib.hx_set_write_codec(self._h, int(codec)))

    def set_bytes_write_codec(self, codec):
        """Writer setting of a Binary store (hx_set_bytes_write_codec):
        CODEC_NONE (default) or CODEC_SNAPPY, the page codec of every SST
        write_bytes, compact and compact_files write from now on."""
        _check(_lib.hx_set_bytes_write_codec(self._h, int(codec)))

    def set_bytes_page_limit(self, limit):
        """Writer setting of a Binary store (hx_set_bytes_page_limit): 0
        (default, one data page per value chunk) or 1 .. 2**30 bytes, the
        size at which write_bytes, compact and compact_files close a data
        page of a value chunk; BYTES_PAGE_LIMIT_REFERENCE is the reference
        writers' 1 MiB."""
        limit = int(limit)
        if not 0 <= limit < 2 ** 32:
            raise HxError(6, "bytes page limit: 0 or 1 .. 2^30")
        _check(_lib.hx_set_bytes_page_limit(self._h, limit))

    def write(self, series, ts, value, enable_check=True, valid=None):
        """ColumnarStorage::write (storage.rs:76-89): stable PK sort + new
        SST + catalog add. Returns the new file's sequence. valid: bool
        array, False = the row's value is null (hx_write_nullable)."""
        series = np.ascontiguousarray(series, dtype=np.uint64)
        ts_a = np.ascontiguousarray(ts, dtype=np.int64)
        value = np.ascontiguousarray(value, dtype=np.float64)
        out = C.c_uint64()
        if valid is not None:
            bits = _validity_bits(valid, len(series))
            _check(_lib.hx_write_nullable(
                self._h, series.ctypes.data_as(C.POINTER(C.c_uint64)),
                ts_a.ctypes.data_as(C.POINTER(C.c_int64)),
                value.ctypes.data_as(C.POINTER(C.c_double)),
                bits.ctypes.data_as(C.POINTER(C.c_uint8)), len(series),
                1 if enable_check else 0, C.byref(out)))
            return out.value
        _check(_lib.hx_write(
            self._h, series.ctypes.data_as(C.POINTER(C.c_uint64)),
            ts_a.ctypes.data_as(C.POINTER(C.c_int64)),
            value.ctypes.data_as(C.POINTER(C.c_double)), len(series),
            1 if enable_check else 0, C.byref(out)))
        return out.value

    def write_bytes(self, series, ts, values, enable_check=True):
        """ColumnarStorage::write for a Binary value column (hx_write_bytes):
        values is a sequence of bytes objects, each below 2^20 bytes.
        Returns the new file's sequence."""
        series = np.ascontiguousarray(series, dtype=np.uint64)
        ts_a = np.ascontiguousarray(ts, dtype=np.int64)
        blob, offs = _bytes_col(values, len(series))
        out = C.c_uint64()
        _check(_lib.hx_write_bytes(
            self._h, series.ctypes.data_as(C.POINTER(C.c_uint64)),
            ts_a.ctypes.data_as(C.POINTER(C.c_int64)), blob.ctypes.data,
            offs.ctypes.data_as(C.POINTER(C.c_int64)), len(series),
            1 if enable_check else 0, C.byref(out)))
        return out.value

    def compact_files(self, input_seqs, devices=None):
        """General compaction of an EXPLICIT input set (executor
        Task{inputs}, keep_builtin): dedups among the named files only;
        the output SST retains per-row __seq__ values."""
        arr = (C.c_uint64 * len(input_seqs))(*input_seqs)
        keep = []
        ds = self._devset(devices, keep)
        seq = C.c_uint64()
        _check(_lib.hx_compact_files(self._h, arr, len(input_seqs),
                                     C.byref(ds) if ds else None,
                                     C.byref(seq)))
        del keep
        return int(seq.value)

    def compact(self, ts_range, devices=None):
        """ColumnarStorage::compact (storage.rs:76-89): GPU-merge the
        ts-overlap closure of the range's SSTs into one new SST. Returns the
        new file's sequence (0 = nothing to compact)."""
        ds = self._devset(devices, [])
        out = C.c_uint64()
        _check(_lib.hx_compact(self._h, _TimeRange(*ts_range),
                               C.byref(ds) if ds else None, C.byref(out)))
        return out.value

    def scan(self, ts_range, series_in=None, projection=None, devices=None,
             batch_limit=None):
        """Streaming parity mode (hx_scan): the merged, deduplicated row
        stream itself — ColumnarStorage::scan semantics (storage.rs:335-370).
        Returns dict of concatenated column arrays in stream order.
        batch_limit: stop the stream (callback returns nonzero — the
        header's early-stop contract) after that many batches."""
        spec, keep = self._spec(ts_range, series_in)
        if projection is not None:
            parr = (C.c_int32 * len(projection))(*projection)
            spec.projection = parr
            spec.n_projection = len(projection)
            keep.append(parr)
        ds = self._devset(devices, keep)
        chunks = []
        valid_parts = []   # per batch: the f64 value column's validity

        _BATCH = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(_ColBatch))

        def on_batch(ctx, bp):
            b = bp.contents
            cols = []
            for i in range(b.n_cols):
                t = b.col_types[i]
                if t == 3:  # Binary value column (hx_bytes_col)
                    bcp = C.cast(b.cols[i], C.POINTER(_BytesCol)).contents
                    offs = np.ctypeslib.as_array(
                        bcp.offsets, shape=(b.n_rows + 1,)).copy()
                    total = int(offs[-1])
                    data = (np.ctypeslib.as_array(
                        bcp.bytes, shape=(total,)).copy()
                        if total else np.empty(0, np.uint8))
                    vals = np.empty(b.n_rows, dtype=object)
                    db = data.tobytes()
                    for r in range(b.n_rows):
                        vals[r] = db[offs[r]:offs[r + 1]]
                    cols.append(vals)
                    continue
                dt = {0: np.uint64, 1: np.int64, 2: np.float64}[t]
                ptr = C.cast(b.cols[i], C.POINTER(C.c_uint64))
                arr = np.ctypeslib.as_array(ptr, shape=(b.n_rows,)).copy()
                cols.append(arr.view(dt))
                if t == 2 and b.validity and b.validity[i]:
                    bits = np.ctypeslib.as_array(
                        b.validity[i], shape=((b.n_rows + 7) // 8,))
                    valid_parts.append(np.unpackbits(
                        bits, bitorder="little")[:b.n_rows].astype(bool))
                elif t == 2:
                    valid_parts.append(np.ones(b.n_rows, dtype=bool))
            chunks.append(cols)
            if batch_limit is not None and len(chunks) >= batch_limit:
                return 1
            return 0

        def on_batch_safe(ctx, bp):
            # exceptions must not cross the C callback boundary
            try:
                return on_batch(ctx, bp)
            except Exception:
                return 1  # stop the stream

        cb = _BATCH(on_batch_safe)
        _check(_lib.hx_scan(self._h, C.byref(spec),
                            C.byref(ds) if ds else None,
                            C.cast(cb, C.c_void_p), None))
        ncols = len(projection) if projection is not None else 3
        names = ["series_id", "timestamp", "value"]
        sel = projection if projection is not None else [0, 1, 2]
        out = {}
        for i in range(ncols):
            parts = [c[i] for c in chunks]
            out[names[sel[i]]] = (np.concatenate(parts) if parts else
                                  np.empty(0))
        # only when the value column carried a bitmap (the store holds null
        # values); values at rows where it is False are unspecified
        if valid_parts and not all(v.all() for v in valid_parts):
            out["value_valid"] = np.concatenate(valid_parts)
        return out


def write_sst_native(path, series, ts, value, seq, row_group=8192):
    """Native C++ SST writer (the compaction output path), exposed for
    tests: writes the reference metric-SST layout without pyarrow."""
    series = np.ascontiguousarray(series, dtype=np.uint64)
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    value = np.ascontiguousarray(value, dtype=np.float64)
    n = len(series)
    _check(_lib.hx_write_sst(
        path.encode(), series.ctypes.data_as(C.POINTER(C.c_uint64)),
        ts.ctypes.data_as(C.POINTER(C.c_int64)),
        value.ctypes.data_as(C.POINTER(C.c_double)), seq, n, row_group))


def _bytes_col(values, n):
    """sequence of n bytes objects -> (uint8 blob, int64 offsets[n + 1])."""
    values = [v if isinstance(v, (bytes, bytearray)) else bytes(v)
              for v in values]
    if len(values) != n:
        raise ValueError("values: one bytes object per row")
    offs = np.zeros(n + 1, dtype=np.int64)
    if n:
        offs[1:] = np.cumsum([len(v) for v in values], dtype=np.int64)
    blob = np.frombuffer(b"".join(values) or b"\0", dtype=np.uint8)
    return blob, offs


def write_sst_native_bytes(path, series, ts, values, seq, seqs=None,
                           row_group=8192, codec=0, page_limit=None):
    """GPU-free writer of one Binary-value SST (hx_write_sst_bytes), rows in
    the order given. seqs: per-row __seq__ values, or None for the constant
    seq. codec: CODEC_NONE (default, the old entry) or CODEC_SNAPPY
    (hx_write_sst_bytes_codec). page_limit: None (the entries above), or the
    data-page limit of the value chunks (hx_write_sst_bytes_paged; 0 = one
    page per chunk)."""
    series = np.ascontiguousarray(series, dtype=np.uint64)
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    n = len(series)
    blob, offs = _bytes_col(values, n)
    sq = None if seqs is None else np.ascontiguousarray(seqs, dtype=np.uint64)
    args = (path.encode(), series.ctypes.data_as(C.POINTER(C.c_uint64)),
            ts.ctypes.data_as(C.POINTER(C.c_int64)), blob.ctypes.data,
            offs.ctypes.data_as(C.POINTER(C.c_int64)),
            None if sq is None else sq.ctypes.data_as(C.POINTER(C.c_uint64)),
            int(seq), n, row_group)
    if page_limit is not None:
        if not 0 <= int(page_limit) < 2 ** 32:
            raise HxError(6, "bytes page limit: 0 or 1 .. 2^30")
        _check(_lib.hx_write_sst_bytes_paged(*args, int(codec),
                                             int(page_limit)))
    elif codec:
        _check(_lib.hx_write_sst_bytes_codec(*args, int(codec)))
    else:
        _check(_lib.hx_write_sst_bytes(*args))


def _ba_pages_call(fn, src, handles, group_start, n_out, row_group, build):
    raw = bytes(src)
    src_a = np.frombuffer(raw or b"\0", dtype=np.uint8)
    handles = np.ascontiguousarray(handles, dtype=np.uint64)
    n_src = len(handles)
    gs = None if group_start is None else \
        np.ascontiguousarray(group_start, dtype=np.uint32)
    if n_out is None:
        n_out = n_src if gs is None else len(gs) - 1
    n_pages = (n_out + row_group - 1) // row_group
    page_off = np.zeros(n_pages + 1, dtype=np.uint64)
    errs, over = C.c_uint64(), C.c_uint64()
    hp = handles.ctypes.data_as(C.POINTER(C.c_uint64)) if n_src else None
    gp = None if gs is None else gs.ctypes.data_as(C.POINTER(C.c_uint32))
    pp = page_off.ctypes.data_as(C.POINTER(C.c_uint64))
    # sizes first (host twin: no GPU), so `out` is exactly the image
    _check(_lib.hx_debug_ba_pages_host(
        src_a.ctypes.data, len(raw), hp, n_src, gp, n_out, row_group, pp,
        None, 0, C.byref(errs), C.byref(over)))
    pages = None
    if build:
        total = int(page_off[-1])
        out = np.full(max(total, 1), 0xA5, dtype=np.uint8)
        _check(fn(src_a.ctypes.data, len(raw), hp, n_src, gp, n_out,
                  row_group, pp, out.ctypes.data, total, C.byref(errs),
                  C.byref(over)))
        pages = [out[int(page_off[g]):int(page_off[g + 1])].tobytes()
                 for g in range(n_pages)]
    return pages, errs.value, over.value


def ba_pages_host(src, handles, group_start=None, n_out=None,
                  row_group=8192, build=True):
    """The host twin of kernel 1f (test hook hx_debug_ba_pages_host; no GPU
    needed). src: bytes; handles: uint64 (off << 20 | len) per source row in
    output order; group_start: n_out + 1 source-row bounds, or None. Returns
    (pages, n_errors, n_over_cap): pages[g] is output row group g's PLAIN
    BYTE_ARRAY page image, refused rows written as empty values."""
    return _ba_pages_call(_lib.hx_debug_ba_pages_host, src, handles,
                          group_start, n_out, row_group, build)


def ba_pages_device(src, handles, group_start=None, n_out=None,
                    row_group=8192, build=True):
    """Kernel 1f through the test hook hx_debug_ba_pages (needs a GPU): the
    production launches over device buffers of exactly the stated sizes.
    Arguments and result as ba_pages_host."""
    return _ba_pages_call(_lib.hx_debug_ba_pages, src, handles, group_start,
                          n_out, row_group, build)


BA_ROW_SKIP = 0x80000000


def _ba_page_minmax_call(fn, values, row_group, skip):
    skip = set(skip)
    n = len(values)
    vals = [b"" if i in skip else bytes(v) for i, v in enumerate(values)]
    row_len = np.array([BA_ROW_SKIP if i in skip else len(v)
                        for i, v in enumerate(vals)], dtype=np.uint32)
    n_pages = (n + row_group - 1) // row_group
    page_off = np.zeros(n_pages + 1, dtype=np.uint64)
    parts = []
    for g in range(n_pages):
        page = b"".join(len(v).to_bytes(4, "little") + v
                        for v in vals[g * row_group:(g + 1) * row_group])
        parts.append(page)
        page_off[g + 1] = page_off[g] + np.uint64(len(page))
    image = np.frombuffer(b"".join(parts), dtype=np.uint8)
    out = np.full(n_pages * 140, 0xA5, dtype=np.uint8)
    _check(fn(image.ctypes.data,
              page_off.ctypes.data_as(C.POINTER(C.c_uint64)),
              row_len.ctypes.data_as(C.POINTER(C.c_uint32)), n, row_group,
              out.ctypes.data))
    res = []
    for g in range(n_pages):
        rec = out[g * 140:(g + 1) * 140]
        has, mn_len, mx_len = (int(x) for x in rec[:12].view(np.uint32))
        mn, mx = rec[12:76].tobytes(), rec[76:140].tobytes()
        if mn_len > 64 or mx_len > 64 or any(mn[mn_len:]) or any(mx[mx_len:]):
            raise AssertionError("BaPageStat record out of form: %r" % (
                (has, mn_len, mx_len, mn, mx),))
        if not has and (mn_len or mx_len):
            raise AssertionError("BaPageStat without statistics has lengths")
        res.append((mn[:mn_len], mx[:mx_len]) if has else None)
    return res


def ba_page_minmax_host(values, row_group=8192, skip=()):
    """The host twin of kernel 1g (test hook hx_debug_ba_page_minmax_host; no
    GPU needed) over the PLAIN BYTE_ARRAY page images of `values` (a sequence
    of bytes), row groups of row_group rows. skip: indices of rows the size
    pass refused (BA_ROW_SKIP): they are empty values in the image. Returns
    one entry per page: (min, max) as bytes, or None when the chunk carries
    no min/max (one of them is longer than 64 bytes)."""
    return _ba_page_minmax_call(_lib.hx_debug_ba_page_minmax_host, values,
                                row_group, skip)


def ba_page_minmax_device(values, row_group=8192, skip=()):
    """Kernel 1g through the test hook hx_debug_ba_page_minmax (needs a GPU):
    the production launch over device buffers of exactly the stated sizes.
    Arguments and result as ba_page_minmax_host."""
    return _ba_page_minmax_call(_lib.hx_debug_ba_page_minmax, values,
                                row_group, skip)


BYTES_PAGE_LIMIT_REFERENCE = 1 << 20
BA_CUT_BATCH = 1024


def _ba_batch_sizes_call(fn, row_len, row_group):
    row_len = np.ascontiguousarray(row_len, dtype=np.uint32)
    n = len(row_len)
    n_rg = (n + row_group - 1) // row_group
    n_b = 0
    if n_rg:
        last = n - (n_rg - 1) * row_group
        n_b = (n_rg - 1) * ((row_group + 1023) // 1024) + (last + 1023) // 1024
    out = np.full(max(n_b, 1), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    _check(fn(row_len.ctypes.data_as(C.POINTER(C.c_uint32)) if n else None,
              n, row_group,
              out.ctypes.data_as(C.POINTER(C.c_uint64)) if n else None))
    return out[:n_b].copy()


def ba_batch_sizes_host(row_len, row_group=8192):
    """The host twin of kernel 1h (hx_debug_ba_batch_sizes_host; no GPU
    needed): the byte sum, 4 + len per row and 4 for a BA_ROW_SKIP row, of
    every 1024-row batch of every row group of row_len (uint32 per row)."""
    return _ba_batch_sizes_call(_lib.hx_debug_ba_batch_sizes_host, row_len,
                                row_group)


def ba_batch_sizes_device(row_len, row_group=8192):
    """Kernel 1h through the test hook hx_debug_ba_batch_sizes (needs a GPU):
    the production launch over device buffers of exactly the stated sizes.
    Arguments and result as ba_batch_sizes_host."""
    return _ba_batch_sizes_call(_lib.hx_debug_ba_batch_sizes, row_len,
                                row_group)


def _validity_bits(valid, n):
    """bool array -> LSB-first bitmap bytes (1 = value present)."""
    valid = np.asarray(valid, dtype=bool)
    if valid.shape != (n,):
        raise ValueError("valid: one bool per row")
    return np.ascontiguousarray(np.packbits(valid, bitorder="little"))


def write_sst_native_nullable(path, series, ts, value, seq, valid=None,
                              row_group=8192):
    """Nullable twin of write_sst_native (hx_write_sst_nullable): `value`
    is written OPTIONAL; valid is a bool array (False = null) or None."""
    series = np.ascontiguousarray(series, dtype=np.uint64)
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    value = np.ascontiguousarray(value, dtype=np.float64)
    n = len(series)
    bits = None if valid is None else _validity_bits(valid, n)
    _check(_lib.hx_write_sst_nullable(
        path.encode(), series.ctypes.data_as(C.POINTER(C.c_uint64)),
        ts.ctypes.data_as(C.POINTER(C.c_int64)),
        value.ctypes.data_as(C.POINTER(C.c_double)),
        None if bits is None else bits.ctypes.data_as(C.POINTER(C.c_uint8)),
        seq, n, row_group))


CODEC_NONE, CODEC_SNAPPY = 0, 1


def write_sst_native_codec(path, series, ts, value, seq, codec, valid=None,
                           nullable=False, row_group=8192):
    """GPU-free writer with a page codec (hx_write_sst_codec). nullable
    declares `value` OPTIONAL (valid: bool array, False = null, or None);
    without it valid must be None."""
    series = np.ascontiguousarray(series, dtype=np.uint64)
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    value = np.ascontiguousarray(value, dtype=np.float64)
    n = len(series)
    bits = None if valid is None else _validity_bits(valid, n)
    _check(_lib.hx_write_sst_codec(
        path.encode(), series.ctypes.data_as(C.POINTER(C.c_uint64)),
        ts.ctypes.data_as(C.POINTER(C.c_int64)),
        value.ctypes.data_as(C.POINTER(C.c_double)),
        None if bits is None else bits.ctypes.data_as(C.POINTER(C.c_uint8)),
        1 if nullable else 0, seq, n, row_group, int(codec)))


def snappy_max_compressed(n):
    """Snappy's bound on the stream of an n-byte page; a smaller output slot
    is refused by the host twin and by kernel 1e."""
    return 32 + n + n // 6


def snappy_compress_host(page, cap=None):
    """The host twin of kernel 1e (test hook hx_debug_snappy_compress_host;
    no GPU needed): the Snappy stream of `page` (bytes-like) as bytes, or
    None when cap (default: the bound) is refused."""
    src = np.frombuffer(bytes(page), dtype=np.uint8)
    n = len(src)
    cap = snappy_max_compressed(n) if cap is None else cap
    dst = np.full(max(cap, 1), 0xA5, dtype=np.uint8)
    size = _lib.hx_debug_snappy_compress_host(
        src.ctypes.data if n else None, n, dst.ctypes.data, cap)
    if size == 0:
        if (dst != 0xA5).any():
            raise RuntimeError("refused call wrote to dst")
        return None
    return dst[:size].tobytes()


def snappy_compress_device(pages, src_align=None, caps=None):
    """Kernel 1e through the test hook hx_debug_snappy_compress (needs a GPU):
    one production launch over `pages` (a list of bytes). src_align: byte
    misalignment 0..63 per page (default 0); caps: output slot size per page
    (default: the bound). Returns (streams, slots, n_errors): streams[i] is
    the page's stream, None for a refused page; slots[i] is its whole output
    slot as the device left it (pre-filled with 0xEE)."""
    n = len(pages)
    lens = np.array([len(p) for p in pages], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    if n:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    blob = np.frombuffer(b"".join(pages) or b"\0", dtype=np.uint8)
    align = np.zeros(n, dtype=np.uint32) if src_align is None else \
        np.ascontiguousarray(src_align, dtype=np.uint32)
    if caps is None:
        caps = [snappy_max_compressed(int(x)) for x in lens]
    out_offs = np.zeros(n + 1, dtype=np.uint64)
    out_offs[1:] = np.cumsum(np.asarray(caps, dtype=np.uint64))
    out = np.zeros(max(int(out_offs[-1]), 1), dtype=np.uint8)
    out_lens = np.zeros(max(n, 1), dtype=np.uint32)
    errs = C.c_uint64()
    _check(_lib.hx_debug_snappy_compress(
        blob.ctypes.data, offs.ctypes.data_as(C.POINTER(C.c_uint64)),
        lens.ctypes.data_as(C.POINTER(C.c_uint32)), n,
        align.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data,
        out_offs.ctypes.data_as(C.POINTER(C.c_uint64)),
        out_lens.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(errs)))
    streams, slots = [], []
    for i in range(n):
        a, b = int(out_offs[i]), int(out_offs[i + 1])
        slots.append(out[a:b].tobytes())
        streams.append(out[a:a + int(out_lens[i])].tobytes()
                       if out_lens[i] else None)
    return streams, slots, errs.value


def pack_optional(values, n, row_group, valid_words=None, valid_bits=None,
                  perm=None):
    """Kernel 1d through the test hook hx_debug_pack_optional (needs a GPU).
    values: the source rows' 8-byte values (any 8-byte dtype); valid_words
    (uint64 0/1 per source row) or valid_bits (LSB-first uint8 bitmap) or
    neither; perm: uint32 source row per output row, or None. Returns
    (packed uint64[n], bitmap uint64[groups * row_group / 64],
    n_valid uint32[groups], n_errors)."""
    values = np.ascontiguousarray(values).view(np.uint64)
    n_src = len(values)
    groups = (n + row_group - 1) // row_group if row_group > 0 else 0
    packed = np.zeros(n, dtype=np.uint64)
    bitmap = np.zeros(groups * (row_group // 64), dtype=np.uint64)
    n_valid = np.zeros(groups, dtype=np.uint32)
    errs = C.c_uint64()
    keep = []

    def ptr(a, dtype, ctype):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ctype))

    _check(_lib.hx_debug_pack_optional(
        values.ctypes.data_as(C.POINTER(C.c_uint64)),
        ptr(valid_words, np.uint64, C.c_uint64),
        ptr(valid_bits, np.uint8, C.c_uint8),
        ptr(perm, np.uint32, C.c_uint32), n_src, n, row_group,
        packed.ctypes.data_as(C.POINTER(C.c_uint64)),
        bitmap.ctypes.data_as(C.POINTER(C.c_uint64)),
        n_valid.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(errs)))
    return packed, bitmap, n_valid, errs.value


def page_levels(path, row_group, column, max_rows=1 << 20):
    """Staging's view of one column chunk's definition levels (test hook
    hx_debug_page_levels; no GPU needed): returns (valid, n_valid,
    level_bytes) where valid is a bool array of the chunk's rows."""
    words = np.zeros((max_rows + 63) // 64, dtype=np.uint64)
    n_rows, n_valid, lvl = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    _check(_lib.hx_debug_page_levels(
        path.encode(), row_group, column.encode(),
        words.ctypes.data_as(C.POINTER(C.c_uint64)), len(words),
        C.byref(n_rows), C.byref(n_valid), C.byref(lvl)))
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    return bits[:n_rows.value].astype(bool), n_valid.value, lvl.value
