# hx_snappy_stored_literal (horaedb_amd/csrc/snappy_stored.h) decides at
# staging time whether a Snappy page is a single stored literal that the scan
# kernels may read in place. The check is a stand-alone C++ program with its
# own main (`make snappy_stored_check`), built with ASan+UBSan when the host
# compiler can link them: exact-fit cases for every literal-length form, one
# byte short/long, preamble mismatches, truncated and over-long preambles, a
# leading copy element, trailing elements, n = 0 and the 4-byte length
# 0xFFFFFFFF. No GPU involved.
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "horaedb_amd", "csrc")


def test_stored_literal_check_program():
    b = subprocess.run(["make", "-C", CSRC, "snappy_stored_check"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(CSRC, "snappy_stored_check")],
                       capture_output=True, text=True)
    print(b.stdout + r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ALL OK"
    assert len(lines) > 50 and not any(ln.endswith("FAIL") for ln in lines)
