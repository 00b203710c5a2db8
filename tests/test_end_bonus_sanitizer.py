"""scripts/end_bonus_sanitize.c, a stand-alone C program with its own main, feeds awfmScoreChainsEndBonus and
awfmAlignChainsEndBonus 2^13 random reads -- enough for the thread pool to cut the batch -- from arrays of exactly their sizes, on 1
and on 16 threads, with B = 0, 5 and 255.  Compiled here with the host sources of the calls and the thread pool under
AddressSanitizer and UBSan, the two runtimes linked statically, and
run as it is, in the environment the test itself has: a read or a write one byte outside any array, or an undefined operation,
stops it.  No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")


def test_host_twins_are_clean_under_the_sanitizers_on_1_and_16_threads(tmp_path):
    exe = str(tmp_path / "end_bonus_sanitize")
    sources = [os.path.join(ROOT, "scripts", "end_bonus_sanitize.c")] + [os.path.join(CSRC, name) for name in (
        "awfm_matrix.c", "awfm_score_affine.c", "awfm_align_affine.c", "awfm_letters.c", "awfm_threads.c")]
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC] + sources +
                          ["-pthread", "-static-libasan", "-static-libubsan", "-o", exe])
    out = subprocess.run([exe], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(b"1 and 16 threads agree") == 2 and b"equal to the matrix calls" in out.stdout and b"end bonus: clean" in out.stdout
    assert b"ERROR" not in out.stderr and b"runtime error" not in out.stderr
