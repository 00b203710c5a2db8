"""examples/read_sam_lines.c is a C program written against the two public headers only (include/AwFmIndex.h, include/awfm_gpu.h):
read_sam.c's pipeline with the slot scores in the place of verification, then awfmSamRecords / awfmGpuSamRecords on the arrays of
the calls before as they are -> a SAM file, header lines and arena written with one fwrite.  It runs the host twins and, where
there is a GPU, the device calls as well (and then refuses to print when the two arenas differ).  Its header is awfmSamHeader's,
and every line passes the parser of tests/sam_records_common.py: the CIGAR's read length is SEQ's, and the text rebuilt from SEQ,
CIGAR and MD is the record's text at POS."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_positions_common as lp  # noqa: E402
import read_candidates_common as rc  # noqa: E402
import sam_records_common as sm  # noqa: E402
import verify_chains_common as vc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND, MIN_VOTES, LOOKBACK, GAP_PENALTY, MAX_OPS, SCORING = 2, 2, 32, 2, 32, (2, 4, 4, 2)


def _compile(tmp_path):
    exe = str(tmp_path / "read_sam_lines")
    lib_dir = os.path.join(ROOT, "avxwindowfmindex_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "read_sam_lines.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lawfmindex_amd", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_read_sam_lines_example_prints_a_sam_file_that_parses(awfm, tmp_path):
    from avxwindowfmindex_amd import _lib
    lengths = lp.record_lengths(43, count=60, longest=900)
    fa = tmp_path / "records.fa"
    records = lp.write_fasta(str(fa), lengths, lp.DNA_LETTERS, 13)
    reads, planted = rc.planted_reads(records, count=24)
    record, at = next(p for p in planted if p is not None)[:2]
    reads.append(records[record][at:at + 50] + records[record][at + 53:at + 110])  # three text characters deleted: one run of D
    reads.append(b"acg")  # shorter than a step: a read without seeds
    reads.append(b"nnnnn" + records[record][at + 5:at + 100] + b"nnnnnnn")  # clipped at both ends
    (tmp_path / "reads.txt").write_bytes(b"\n".join(reads) + b"\n")
    args = [str(rc.E2E_STEP), str(rc.E2E_MIN_LENGTH), str(rc.E2E_CAP), str(rc.E2E_MAX_HITS), str(BAND), str(MIN_VOTES), str(LOOKBACK), str(GAP_PENALTY),
            str(vc.E2E_W), str(vc.E2E_X), str(MAX_OPS)] + [str(v) for v in SCORING]
    out = subprocess.run([_compile(tmp_path), "records.fa", "reads.txt"] + args, cwd=tmp_path, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "check.awfmi"))
    try:
        header = awfm.sam_header(ix)
        name_offsets, name_chars = awfm.record_names(ix)
        names = {name: records[i] for i, name in enumerate(awfm.strings_of(name_offsets, name_chars))}
    finally:
        ix.dealloc()
    assert header.count(b"@SQ") == len(records) == len(names) and out.stdout.startswith(header)
    lines = out.stdout[len(header):].splitlines(keepends=True)
    assert len(lines) == len(reads)
    aligned = 0
    for r, (line, read) in enumerate(zip(lines, reads)):
        rec = sm.parse(line)
        assert rec["qname"] == b"%d" % r and rec["seq"] == read and rec["qual"] == b"*" and rec["rnext"] == b"*" and rec["pnext"] == rec["tlen"] == 0
        if rec["flag"] & 0x4:
            assert rec["flag"] == 4 and (rec["rname"], rec["pos"], rec["mapq"], rec["cigar"], rec["tags"]) == (b"*", 0, 0, b"*", {})
            continue
        aligned += 1
        assert rec["flag"] == 0 and 0 <= rec["mapq"] <= 60 and set(rec["tags"]) == {"NM", "AS", "XS", "MD"} and rec["tags"]["AS"] > rec["tags"]["XS"] >= 0
        under = sm.text_under(rec["seq"], rec["cigar"], rec["tags"]["MD"])
        assert names[rec["rname"]][rec["pos"] - 1:rec["pos"] - 1 + len(under)].upper() == under, (r, line)
    assert aligned >= sum(p is not None for p in planted) + 2 and sm.parse(lines[-2])["flag"] == 4  # the read without seeds
    last = sm.parse(lines[-1])
    assert (last["pos"], last["cigar"], last["tags"]["MD"], last["tags"]["NM"]) == (at + 5 + 1, b"5S95M7S", b"95", 0)  # one clips
    assert any(b"D" in sm.parse(x)["cigar"] for x in lines)
    side = "device" if _lib.lib().awfmGpuDeviceCount() > 0 else "host"
    assert f"reads {len(reads)} ".encode() in out.stderr and f"aligned {aligned} unaligned {len(reads) - aligned} ".encode() in out.stderr
    assert f"bytes {len(out.stdout)} on the {side}".encode() in out.stderr
