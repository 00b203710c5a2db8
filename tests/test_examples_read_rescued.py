"""examples/read_rescued.c is a C program written against the two public headers only (include/AwFmIndex.h, include/awfm_gpu.h):
read_clipped.c for mate 1 of every pair, then awfmScoreWindowsAffine / awfmGpuScoreWindowsAffine for mate 2 in the window
[mate 1's textBegin, + width) of mate 1's sequence, then awfmAlignChainsAffine / awfmGpuAlignChainsAffine on the slot that call
wrote -> one line `pair header pos1 score1 CIGAR1 pos2 windowScore score2 CIGAR2` per pair.  It runs the host twins and, where
there is a GPU, the device calls as well (and then refuses to print when the two differ); its lines must be what the Python API
gives on the same FASTA file: the host's pipeline for mate 1 as in tests/test_examples_read_clipped.py, score_windows_affine and
align_chains_affine_host for mate 2.  Mate 2 carries a substitution at every 11th character: the seeds could not place it."""
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import local_positions_common as lp  # noqa: E402
import read_candidates_common as rc  # noqa: E402
import read_chains_common as ch  # noqa: E402
import verify_chains_common as vc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND, MIN_VOTES, SLOTS, LOOKBACK, GAP_PENALTY, MAX_OPS, SCORING, WIDTH, MIN_SCORE = 2, 2, 4, 32, 2, 24, (1, 4, 6, 1), 400, 30
SWAP = {ord("a"): ord("c"), ord("c"): ord("g"), ord("g"): ord("t"), ord("t"): ord("a")}


def _compile(tmp_path):
    exe = str(tmp_path / "read_rescued")
    lib_dir = os.path.join(ROOT, "avxwindowfmindex_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "read_rescued.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lawfmindex_amd",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_read_rescued_example_prints_what_the_python_api_finds(awfm, tmp_path):
    from avxwindowfmindex_amd import _lib
    rng = np.random.default_rng(17)
    fa = tmp_path / "records.fa"
    records = lp.write_fasta(str(fa), [900, 0, 1300, 5, 700], lp.DNA_LETTERS, 13)
    mates1, mates2, planted = [], [], []
    for _ in range(20):
        s = int(rng.choice([0, 2, 4]))
        p = int(rng.integers(0, len(records[s]) - 300))
        mate = bytearray(records[s][p + 160:p + 260])
        for k in range(5, 100, 11):
            mate[k] = SWAP[mate[k] | 0x20]
        mates1.append(records[s][p:p + 100])
        mates2.append(bytes(mate))
        planted.append((s, p))
    mates1 += [b"acg", records[4][-90:]]       # a mate 1 without seeds: its pair is not looked at; and one whose window leaves the record
    mates2 += [records[0][:50], records[0][:60]]  # (a mate 2 that lies elsewhere: nothing worth minScore in the window)
    (tmp_path / "pairs.txt").write_bytes(b"".join(a + b"\n" + b + b"\n" for a, b in zip(mates1, mates2)))
    args = [str(WIDTH), str(rc.E2E_STEP), str(rc.E2E_MIN_LENGTH), str(rc.E2E_CAP), str(rc.E2E_MAX_HITS), str(BAND), str(MIN_VOTES), str(LOOKBACK),
            str(GAP_PENALTY), str(vc.E2E_W), str(vc.E2E_X), str(MAX_OPS)] + [str(v) for v in SCORING] + [str(MIN_SCORE)]
    out = subprocess.run([_compile(tmp_path), "records.fa", "pairs.txt"] + args, cwd=tmp_path, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    # mate 1 by the host's pipeline, as tests/test_examples_read_clipped.py does it
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "check.awfmi"))
    inst = rc.host_pipeline(awfm, ix, mates1)
    case = ch.candidate_case(awfm, inst, BAND, SLOTS, max_hits_per_seed=rc.E2E_MAX_HITS, min_votes=MIN_VOTES)
    got = case.host(awfm, max_hits_per_seed=rc.E2E_MAX_HITS, band=BAND, lookback=LOOKBACK, gap_penalty=GAP_PENALTY)
    text, ends = vc.text_of(records)
    slots = dict({name: got[name] for name in vc.SLOT_FIELDS[1:]}, sequences=case.sequences)
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in mates1])))
    verified = vc.Case(b"".join(mates1), offsets, slots, text.tobytes(), ends).host(awfm, vc.E2E_W, vc.E2E_X)
    first = awfm.align_chains_affine_host(b"".join(mates1), offsets, slots, verified["bestSlots"], text.tobytes(), ends, band_pad=vc.E2E_W,
                                          max_drift=vc.E2E_X, scoring=SCORING, max_ops=MAX_OPS)
    n = len(mates1)
    has = np.array([0 < int(v) < af.TOO_LONG for v in first["scores"]])
    sequences = np.array([int(case.sequences[r, int(verified["bestSlots"][r])]) if has[r] else 0xFFFFFFFF for r in range(n)], np.uint32)
    begins = np.where(has, first["textBegins"], 0).astype(np.uint64)
    # mate 2 by the window call and affine alignment on the slot it wrote
    mate_offsets = np.concatenate(([0], np.cumsum([len(r) for r in mates2])))
    placed = awfm.score_windows_affine(b"".join(mates2), mate_offsets, sequences, begins, np.where(has, begins + np.uint64(WIDTH), 0), text.tobytes(), ends,
                                       scoring=SCORING, min_score=MIN_SCORE)
    second = awfm.align_chains_affine_host(b"".join(mates2), mate_offsets, {name: placed[name] for name in vc.SLOT_FIELDS}, np.zeros(n, np.uint32),
                                           text.tobytes(), ends, band_pad=vc.E2E_W, max_drift=vc.E2E_X, scoring=SCORING, max_ops=MAX_OPS)

    def script(aligned, r, present):
        k = int(aligned["numOps"][r])
        return (awfm.cigar_of(aligned["ops"][r][:k]) if present and 0 < k <= MAX_OPS else "*").encode()

    want, rescued = [], 0
    for r in range(n):
        if not has[r]:
            want.append(b"%d\t*\t0\t0\t*\t0\t0\t0\t*" % r)
            continue
        ok = 0 < int(second["scores"][r]) < af.TOO_LONG
        rescued += ok
        window_score = int(placed["scores"][r]) if int(placed["scores"][r]) < af.TOO_LONG else 0
        want.append(b"%d\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%s" % (r, ix.header(int(sequences[r])), int(first["textBegins"][r]), int(first["scores"][r]),
                                                            script(first, r, True), int(second["textBegins"][r]) if ok else 0, window_score,
                                                            int(second["scores"][r]) if ok else 0, script(second, r, ok)))
    # EVERY planted mate 2 is rescued at its planted place with the window's score; the two odd pairs are not
    for r, (s, p) in enumerate(planted):
        fields = want[r].split(b"\t")
        assert fields[1] == ix.header(s) and int(fields[2]) == p and int(fields[5]) == p + 160 and fields[6] == fields[7] and int(fields[7]) >= 50, want[r]
        assert fields[8] == b"5=1X10=1X10=1X10=1X10=1X10=1X10=1X10=1X10=1X6=", want[r]
    assert rescued == len(planted) and want[-2] == b"%d\t*\t0\t0\t*\t0\t0\t0\t*" % (n - 2) and want[-1].endswith(b"\t0\t*") and not want[-1].startswith(b"%d\t*" % (n - 1))
    assert out.stdout.split(b"\n")[:-1] == want
    side = "device" if _lib.lib().awfmGpuDeviceCount() > 0 else "host"
    assert (f"pairs {n} windows {inst.num_seeds} aligned {int(has.sum())} found {placed['numFound']} rescued {rescued} on the {side}").encode() in out.stderr
    ix.dealloc()
