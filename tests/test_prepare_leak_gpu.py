# A refused hx_prepare frees what it had built. hx_prepare stages its plans
# one after the other, so a store whose second plan is refused (a gzip file)
# has already uploaded the first plan's blob by then. Prepared twice over the
# same card (devices=[0, 0] gives two plans; ids are validated by range only)
# the larger, valid file lands on plan 0 and the gzip file on plan 1.
#
# Only the device half of the leak is observable cheaply: free device memory
# before and after, read with hipMemGetInfo from the HIP runtime the library
# itself has loaded (what torch.cuda.mem_get_info reports, without bringing up
# a second runtime inside the process). The pinned host blob of the refused
# plan is released by the same single mechanism — the deleter of the
# unique_ptr that owns the hx_prepared — so it is covered by this test only
# through that.
import ctypes

import numpy as np
import pytest

from horaedb_amd import AGG_COUNT, HxError, Store, lib_path
from tools.gen_ssts import write_sst

pytestmark = pytest.mark.gpu

UNSUPPORTED = 3
FULL = (0, 2**62)


def _free_device_bytes():
    # looked up through the library's own handle: dlsym follows its
    # dependencies, so this is the runtime that did the allocations even when
    # another copy (torch's) is loaded in the process
    hip = ctypes.CDLL(lib_path())
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipSetDevice(0) == 0 and hip.hipDeviceSynchronize() == 0
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_refused_prepare_frees_device_memory(tmp_path):
    ddir = tmp_path / "data"
    ddir.mkdir()
    n_big, n_small = 2_000_000, 10_000
    rng = np.random.default_rng(11)
    big = str(ddir / "1.sst")
    write_sst(big, np.arange(n_big, dtype=np.uint64) // 4,
              np.arange(n_big, dtype=np.int64) % 4, rng.random(n_big), 1)
    write_sst(str(ddir / "2.sst"), np.arange(n_small, dtype=np.uint64),
              np.full(n_small, 1_000_000, dtype=np.int64),
              rng.random(n_small), 2, compression="gzip")

    def scan_valid(st):
        with st.prepare(FULL, devices=[0], sst_subset=[(big, 1)]) as p:
            res = p.exec_agg(ops=AGG_COUNT)
            assert int(res["count"].sum()) == n_big
            return p.stats()["bytes_staged"]

    with Store(str(tmp_path)) as st:
        staged = scan_valid(st)   # also warms every one-time allocation
        assert staged >= n_big * 24
        free_before = _free_device_bytes()
        for _ in range(3):
            with pytest.raises(HxError) as ei:
                st.prepare(FULL, devices=[0, 0])
            assert ei.value.code == UNSUPPORTED
            assert "codec" in str(ei.value)
        lost = free_before - _free_device_bytes()
        print(f"staged {staged} B per valid prepare; {lost} B of device "
              f"memory lost over three refused prepares")
        assert lost < staged
        assert scan_valid(st) == staged   # the handle still works
