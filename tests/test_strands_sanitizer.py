"""scripts/strands_sanitize.c, a stand-alone C program with its own main, feeds awfmChooseStrands pairs written out by hand -- a proper
pair from either strand, bests on one strand, one mate placed, none, a malformed read, windows raised to 0 --, paired and
unpaired, from heap blocks of exactly the arrays' sizes, then 2^12 random reads at 1, 5 and 16 slots a row on 1 and on 16
threads, and awfmOrientReads every read length 0 to 70 with malformed reads and a capacity that cuts the last read.  Compiled here
with csrc/awfm_strands.c and the thread pool under AddressSanitizer and UBSan, the two runtimes linked statically, and run as it
is, in the environment the test itself has: a read or a write one byte outside any array, or an undefined operation, stops it.
No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")


def test_host_twins_are_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "strands_sanitize")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "scripts", "strands_sanitize.c"), os.path.join(CSRC, "awfm_strands.c"),
                           os.path.join(CSRC, "awfm_threads.c"), "-pthread", "-static-libasan", "-static-libubsan", "-o", exe])
    out = subprocess.run([exe], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert b"hand-written pairs, paired and unpaired: as expected" in out.stdout and b"random tables: 1 and 16 threads agree" in out.stdout
    assert b"orient on exact blocks: as expected" in out.stdout and b"ERROR" not in out.stderr and b"runtime error" not in out.stderr
