"""scripts/sam_records_sanitize.c, a stand-alone C program with its own main, feeds awfmSamRecords lines written out by hand -- pairs
in every combination, every reason a read is unaligned, every optional array NULL -- from heap blocks of exactly the arrays' sizes,
then 2^13 random reads -- enough for the thread pool to cut the batch -- on 1 and on 16 threads, and awfmRecordNames and
awfmSamHeader at every capacity.  Compiled here with csrc/awfm_sam.c and the thread pool under AddressSanitizer and UBSan, the two
runtimes linked statically, and run as it is, in the environment the test itself has: a read or a write one byte outside any
array, or an undefined operation, stops it.  No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")


def test_host_twin_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "sam_records_sanitize")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "scripts", "sam_records_sanitize.c"), os.path.join(CSRC, "awfm_sam.c"),
                           os.path.join(CSRC, "awfm_threads.c"), "-pthread", "-static-libasan", "-static-libubsan", "-o", exe])
    out = subprocess.run([exe], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(b"three capacities: as expected") == 2 and b"1 and 16 threads agree" in out.stdout
    assert b"names and header of 4 records at every capacity: as expected" in out.stdout and b"ERROR" not in out.stderr and b"runtime error" not in out.stderr
