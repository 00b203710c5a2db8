"""awfmGpuAlignmentStrings (include/awfm_gpu.h "alignment strings", csrc/awfm_strings_kernel.h) against its host twin
awfmAlignmentStrings, which tests/test_alignment_strings.py pins to the plain-Python restatement of the definition and to its hand
values -- and against that restatement itself, so that the twin is not the only witness: every output, byte for byte, on the
edge lists at the natural tier and with strings_tier=direct, on 1 to 129 reads with empty reads at the edges of a wave, on spans
of exactly the LDS tile and one byte more, beside a D of 5000 positions and a read of 4096 runs, at maxOps of both load widths,
with the arenas skewed against a dword boundary, at capacities that cut the output, on 2^12 reads in both alphabets, from two
streams at once, without a text, with every output NULL in turn, and end to end from a FASTA file behind both alignment calls.
Inputs, outputs and the scratch (exactly its declared size) lie between guard words."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alignment_strings_common as sc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 64, 0xA5
NAMES = ("cigarOffsets", "cigarChars", "mdOffsets", "mdChars", "numSkipped", "numOverflow")
TILE = 8192  # kStringsTileBytes


def _guarded(torch, array, skew=0):
    """the array's bytes on the device between guard words, `skew` bytes further in -> (buffer, address)"""
    raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
    host = np.concatenate((np.full(GUARD + skew, PATTERN, np.uint8), raw, np.full(GUARD, PATTERN, np.uint8)))
    buffer = torch.from_numpy(host).to("cuda")
    return buffer, buffer.data_ptr() + GUARD + skew


class Image:
    """an image whose index is built from a well-formed text of the case's length, with the case's byte-rich text and its record
    table installed: the call takes the image for its text, record table and alphabet only"""

    def __init__(self, awfm, case, text=True):
        letters = np.frombuffer(b"acgt" if case.alphabet == sc.DNA else b"acdefghiklmnpqrstvwy", np.uint8)
        well_formed = letters[np.random.default_rng(7).integers(0, letters.size, len(case.text))]
        self.ix = awfm.create_index(well_formed, case.alphabet, 2, 2)
        self.g = awfm.GpuIndex(self.ix)
        if text:
            self.g.set_text(case.text)
        if case.ends is not None:
            self.g.set_record_table(case.ends)

    def close(self):
        self.g.destroy()
        self.ix.dealloc()


class Scratch:
    """exactly awfmGpuAlignmentStringsScratchBytes bytes between guard words"""

    def __init__(self, torch, g, num_reads):
        self.size = g.alignment_strings_scratch_bytes(num_reads)
        assert self.size > 8 * num_reads
        self.buffer = torch.full((self.size + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        self.address = self.buffer.data_ptr() + GUARD
        assert self.address % 16 == 0

    def check(self):
        raw = self.buffer.cpu().numpy()
        assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + self.size:] == PATTERN).all(), "wrote outside the scratch"


class DeviceCall:
    """the arrays of one case on the device between guard words -- ops_shift: the rows 4, 8 or 12 bytes off a 16-byte boundary --
    and guarded outputs for calls on them"""

    def __init__(self, awfm, torch, case, ops_shift=0):
        self.awfm, self.torch, self.case = awfm, torch, case
        arrays = case.arrays()
        self.buffers = {name: _guarded(torch, a, skew=ops_shift if name == "ops" else 0) for name, a in arrays.items()}
        self.inputs = awfm.string_inputs(*(self.buffers[name][1] for name in ("sequences", "slots", "text_begins", "num_ops", "ops")))

    def run(self, g, scratch, classic=False, cigar_capacity=None, md_capacity=None, outputs=None, skew=0, stream=0, skipped_before=0,
            overflow_before=0, launch=True, want=None):
        torch, n = self.torch, self.case.num_reads
        outputs = list(NAMES) if outputs is None else list(outputs)
        if cigar_capacity is None or md_capacity is None:
            totals = sc.expected(self.case, classic) if want is None else want
            cigar_capacity = int(totals["cigarOffsets"][-1]) if cigar_capacity is None else cigar_capacity
            md_capacity = int(totals["mdOffsets"][-1]) if md_capacity is None else md_capacity
        sizes = dict(cigarOffsets=8 * (n + 1), cigarChars=cigar_capacity, mdOffsets=8 * (n + 1), mdChars=md_capacity, numSkipped=8, numOverflow=8)
        skews = dict(cigarChars=skew, mdChars=(4 - skew) % 4 if skew else 0)  # (the two arenas at different residues)
        buffers = {name: torch.full((sizes[name] + 2 * GUARD + 4,), PATTERN, dtype=torch.uint8, device="cuda") for name in outputs}
        at = {name: GUARD + skews.get(name, 0) for name in outputs}
        for name, before in (("numSkipped", skipped_before), ("numOverflow", overflow_before)):
            if name in outputs:
                buffers[name][GUARD:GUARD + 8] = torch.from_numpy(np.array([before], np.uint64).view(np.uint8)).to("cuda")
        sout = self.awfm.string_outputs(cigarCapacity=cigar_capacity, mdCapacity=md_capacity,
                                        **{name: b.data_ptr() + at[name] for name, b in buffers.items()})
        torch.cuda.synchronize()

        def enqueue():
            g.alignment_strings(self.inputs, n, sout, scratch.address, max_candidates=self.case.C, max_ops=self.case.max_ops, classic=classic,
                                stream=stream)

        def collect():
            result = {}
            for name, b in buffers.items():
                raw, size = b.cpu().numpy(), sizes[name]
                assert (raw[:at[name]] == PATTERN).all() and (raw[at[name] + size:] == PATTERN).all(), f"wrote outside {name}"
                body = raw[at[name]:at[name] + size].copy()
                result[name] = int(body.view(np.uint64)[0]) if name.startswith("num") else body.view(np.uint64) if name.endswith("Offsets") else body
            for name, (buffer, address) in self.buffers.items():
                raw = buffer.cpu().numpy()
                begin = address - buffer.data_ptr()
                assert (raw[:begin] == PATTERN).all() and (raw[-GUARD:] == PATTERN).all(), f"wrote beside the input {name}"
            scratch.check()
            return result

        if launch:
            enqueue()
        return (None if launch else enqueue), collect

    def __call__(self, *args, **kwargs):
        _, collect = self.run(*args, **kwargs)
        self.torch.cuda.synchronize()
        return collect()


def host(awfm, case, **arguments):
    return awfm.alignment_strings_host(text=case.text, sequence_ends=case.ends, alphabet=case.alphabet, fill=PATTERN, **case.arrays(), **arguments)


def check(awfm, torch, g, case, what="", ops_shift=0, **arguments):
    """one device call against the twin and the restatement, every output -> the device's result"""
    classic = arguments.get("classic", False)
    names = arguments.get("outputs")
    twin = host(awfm, case, **{k: v for k, v in arguments.items() if k != "skew"})
    restated = sc.expected(case, classic, arguments.get("cigar_capacity"), arguments.get("md_capacity"), fill=PATTERN,
                           skipped_before=arguments.get("skipped_before", 0), overflow_before=arguments.get("overflow_before", 0),
                           cigar_arena=names is None or "cigarChars" in names, md_arena=names is None or "mdChars" in names)
    got = DeviceCall(awfm, torch, case, ops_shift)(g, Scratch(torch, g, case.num_reads), want=restated if arguments.get("cigar_capacity") is None else None,
                                                   **arguments)
    compare = NAMES if names is None else names
    assert sorted(got) == sorted(compare)
    sc.assert_same(got, twin, names=compare, what=(what, "twin"))
    sc.assert_same(got, restated, names=compare, what=(what, "restatement"))
    return got


@pytest.mark.parametrize("tier", [None, "direct"], ids=["natural", "direct"])
def test_edge_lists_equal_the_host_twin_and_the_restatement(awfm, require_gpu, diag, tier):
    import torch
    diag(strings_tier=tier)
    for alphabet in (sc.DNA, sc.AMINO):
        hand, edges, (skipped, which) = sc.hand_case(), sc.edge_case(alphabet), sc.skipped_case(alphabet)
        for case, name in ((hand, "hand"), (edges, "edges"), (skipped, "skipped")):
            if name == "hand" and alphabet == sc.AMINO:
                continue
            image = Image(awfm, case)
            try:
                for classic in (False, True):
                    got = check(awfm, torch, image.g, case, what=(name, alphabet, classic), classic=classic, skipped_before=5, overflow_before=2)
                    assert got["numOverflow"] == 2 and got["numSkipped"] == 5 + (len(which) if name == "skipped" else 0)
                    if name == "hand":
                        assert awfm.strings_of(got["cigarOffsets"], got["cigarChars"]) == [h[4] if classic else h[3] for h in sc.HAND]
                        assert awfm.strings_of(got["mdOffsets"], got["mdChars"]) == [h[5] for h in sc.HAND]
            finally:
                image.close()


def _with_empty_edges(case, seed):
    """the reads at the first and the last place of every wave become NONE and SKIPPED in turn"""
    reads = list(case.reads)
    places = sorted({p for p in [0, 63, 64, 127, 128, len(reads) - 1] if p < len(reads)})
    for i, p in enumerate(places):
        reads[p] = sc.Read(num_ops=0, slot=sc.NO_SLOT) if (i + seed) % 2 == 0 else sc.Read(0, 0, sc.script("3= 1X"), slot=case.C)
    return sc.Case(reads, case.text, case.ends, case.alphabet, C=case.C, max_ops=case.max_ops)


@pytest.mark.parametrize("tier", [None, "direct"], ids=["natural", "direct"])
def test_read_counts_around_a_wave_load_widths_skews_and_capacities(awfm, require_gpu, diag, tier):
    import torch
    diag(strings_tier=tier)
    base = sc.random_case(41, 129, sc.DNA, C=3, max_ops=32, text_length=1 << 12, num_records=3)
    image = Image(awfm, base)
    try:
        g = image.g
        for n in (1, 63, 64, 65, 129):
            cut = sc.Case(base.reads[:n], base.text, base.ends, base.alphabet, C=base.C, max_ops=base.max_ops)
            check(awfm, torch, g, cut, what=("reads", n), classic=bool(n & 1))
            for seed in (0, 1):
                check(awfm, torch, g, _with_empty_edges(cut, seed), what=("empty edges", n, seed))
        for max_ops in (1, 3, 4, 32):  # dword loads of the rows, and 16-byte loads
            case = sc.random_case(42 + max_ops, 200, sc.DNA, C=2, max_ops=max_ops, like=base)
            check(awfm, torch, g, case, what=("maxOps", max_ops), classic=True)
            if max_ops % 4 == 0:  # rows that are whole 16-byte pieces, but not on a 16-byte boundary
                check(awfm, torch, g, case, what=("maxOps", max_ops, "rows off the boundary"), ops_shift=4)
        # spans begin and end at every residue mod 4: reads whose strings have every length from 2 on, at every skew of the arenas
        runs = [[(1, sc.EQ)] + [(1, sc.X)] * (i % 7) + [(3, sc.D)] * (i % 3) + [(10 ** (i % 4), sc.EQ)] for i in range(150)]
        longest = max(range(3), key=lambda s: base.record_bounds(s)[1] - base.record_bounds(s)[0])  # (of more than 4096 / 3 positions)
        lengths = sc.Case([sc.Read(longest, i, r) for i, r in enumerate(runs)], base.text, base.ends, sc.DNA, C=1, max_ops=12)
        assert sc.expected(lengths)["numSkipped"] == 0
        spans = sc.expected(lengths)
        for name in ("cigarOffsets", "mdOffsets"):
            assert {int(v) % 4 for v in spans[name][::64]} | {int(v) % 4 for v in spans[name][1:]} == {0, 1, 2, 3}
        for skew in (0, 1, 2, 3):
            check(awfm, torch, g, lengths, what=("skew", skew), skew=skew)
            for first in (1, 2, 3):  # and the first wave's span ends at every residue as well
                shifted = sc.Case(lengths.reads[first:], base.text, base.ends, sc.DNA, C=1, max_ops=12)
                check(awfm, torch, g, shifted, what=("skew", skew, "from", first), skew=skew, classic=True)
        # capacities: the total, one less, a cut through the middle of the second wave's span, 0 -- the two arenas independently
        totals = int(spans["cigarOffsets"][-1]), int(spans["mdOffsets"][-1])
        middle = (int(spans["cigarOffsets"][100]) + int(spans["cigarOffsets"][101])) // 2, (int(spans["mdOffsets"][90]) + int(spans["mdOffsets"][91])) // 2
        assert spans["cigarOffsets"][100] < middle[0] < spans["cigarOffsets"][101] and spans["mdOffsets"][90] < middle[1] < spans["mdOffsets"][91]
        for cigar_capacity, md_capacity in ((totals[0] - 1, totals[1]), (totals[0], totals[1] - 1), (middle[0], totals[1] + 3), (totals[0] + 1, middle[1]),
                                            (middle[0], middle[1]), (0, totals[1]), (totals[0], 0), (0, 0)):
            for skew in (0, 3):
                got = check(awfm, torch, g, lengths, what=("capacity", cigar_capacity, md_capacity), cigar_capacity=cigar_capacity, md_capacity=md_capacity,
                            skew=skew, overflow_before=11)
                assert got["numOverflow"] > 11
        # every output NULL in turn (an offsets array with its arena), and alone (but an arena)
        for name in NAMES:
            missing = [m for m in NAMES if m != name and not (name.endswith("Offsets") and m == name[:-7] + "Chars")]
            check(awfm, torch, g, lengths, what=("without", name), outputs=missing, cigar_capacity=totals[0], md_capacity=totals[1], skipped_before=3)
            if not name.endswith("Chars"):
                check(awfm, torch, g, lengths, what=("only", name), outputs=[name], cigar_capacity=totals[0], md_capacity=totals[1], overflow_before=4)
        check(awfm, torch, g, lengths, what="no output", outputs=[], cigar_capacity=0, md_capacity=0)
    finally:
        image.close()


def _tile_case(extra):
    """192 reads: the CIGARs of the first wave and the MDs of the second fill exactly the LDS tile, or `extra` bytes more"""
    text = bytes(np.random.default_rng(3).choice(np.frombuffer(b"ACGTacgtn", np.uint8), 600))
    alternating = [(1, sc.EQ), (1, sc.X)] * 32  # 64 runs of two bytes: a CIGAR of 128 bytes, an MD of 32 * 2 + 1
    wave0 = [sc.Read(0, r, alternating) for r in range(64)]
    wave1 = [sc.Read(0, r, [(125, sc.D)]) for r in range(64)]  # 0^, 125 letters, 0: an MD of 128 bytes
    wave2 = [sc.Read(0, r, sc.script("5= 1X 2I 3=")) for r in range(64)]
    if extra:
        wave0[17] = sc.Read(0, 17, [(10, sc.EQ)] + alternating[1:])
        wave1[63] = sc.Read(0, 63, [(126, sc.D)])
    case = sc.Case(wave0 + wave1 + wave2, text, None, sc.DNA, C=1, max_ops=64)
    spans = sc.expected(case)
    assert int(spans["cigarOffsets"][64]) == TILE + extra and int(spans["mdOffsets"][128]) - int(spans["mdOffsets"][64]) == TILE + extra
    return case


def test_spans_of_exactly_the_tile_and_one_byte_more(awfm, require_gpu):
    import torch
    kernel = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "avxwindowfmindex_amd", "csrc", "awfm_strings_kernel.h")).read()
    assert f"constexpr unsigned kStringsTileBytes = {TILE};" in kernel
    image = Image(awfm, _tile_case(0))
    try:
        for extra in (0, 1):
            for skew in (0, 1, 3):
                check(awfm, torch, image.g, _tile_case(extra), what=("tile", extra, skew), skew=skew)
    finally:
        image.close()


def test_a_long_deletion_and_a_read_of_4096_runs_among_short_reads(awfm, require_gpu):
    import torch
    rng = np.random.default_rng(8)
    text = sc.random_text(rng, 1 << 14, sc.DNA)
    short = lambda r: sc.Read(0, 3 * r, sc.script("4= 1X 2= 1D 6="))  # noqa: E731
    reads = [short(r) for r in range(70)]
    reads[20] = sc.Read(0, 100, [(3, sc.EQ), (5000, sc.D), (2, sc.EQ)])
    case = sc.Case(reads, text, None, sc.DNA, C=1, max_ops=8)
    image = Image(awfm, case)
    try:
        got = check(awfm, torch, image.g, case, what="a D of 5000")
        assert int(got["mdOffsets"][21]) - int(got["mdOffsets"][20]) == 1 + 1 + 5000 + 1
        many = [(1 + i % 2, (sc.EQ, sc.X, sc.EQ, sc.I)[i % 4]) for i in range(sc.MAX_OPS)]
        reads = [sc.Read(0, r, sc.script("4= 1X")) for r in range(66)]
        reads[40] = sc.Read(0, 9, many)
        case = sc.Case(reads, text, None, sc.DNA, C=1, max_ops=sc.MAX_OPS)
        for classic in (False, True):
            got = check(awfm, torch, image.g, case, what=("4096 runs", classic), classic=classic)
            assert int(got["cigarOffsets"][41]) - int(got["cigarOffsets"][40]) == (2 * sc.MAX_OPS if not classic else len(sc.expected(case, True)["strings"][40][0]))
    finally:
        image.close()


@pytest.mark.parametrize("alphabet", [sc.DNA, sc.AMINO], ids=["dna", "amino"])
def test_a_batch_of_4096_reads(awfm, require_gpu, alphabet):
    import torch
    case = sc.random_case(50 + alphabet, 1 << 12, alphabet, C=4, max_ops=32, text_length=1 << 15, num_records=9)
    image = Image(awfm, case)
    try:
        for classic in (False, True):
            got = check(awfm, torch, image.g, case, what=("4096 reads", classic), classic=classic)
            assert 0 < got["numSkipped"] < 600 and got["numOverflow"] == 0
    finally:
        image.close()


def test_without_a_text_bad_arguments_and_two_streams_with_a_scratch_each(awfm, require_gpu):
    import torch
    a = sc.random_case(61, 700, sc.DNA, C=4, max_ops=32)
    b = sc.random_case(62, 500, sc.DNA, C=3, max_ops=7, like=a)
    image = Image(awfm, a, text=False)
    try:
        g = image.g
        calls = [DeviceCall(awfm, torch, a), DeviceCall(awfm, torch, b)]
        scratches = [Scratch(torch, g, a.num_reads), Scratch(torch, g, b.num_reads)]
        want = [sc.expected(a, False, fill=PATTERN), sc.expected(b, True, fill=PATTERN)]
        twins = [host(awfm, a), host(awfm, b, classic=True)]
        # without a text: AwFmUnsupportedVersionError, and nothing is written
        enqueue, collect = calls[0].run(g, scratches[0], launch=False, want=want[0])
        with pytest.raises(awfm.AwFmError) as e:
            enqueue()
        assert e.value.rc == awfm.AwFmUnsupportedVersionError
        torch.cuda.synchronize()
        untouched = collect()
        assert all((np.asarray(untouched[name]).view(np.uint8) == PATTERN).all() for name in NAMES[:4]) and untouched["numSkipped"] == 0
        assert (scratches[0].buffer.cpu().numpy() == PATTERN).all()
        g.set_text(a.text)
        offsets = torch.full((8 * (a.num_reads + 1),), PATTERN, dtype=torch.uint8, device="cuda")
        some = awfm.string_outputs(cigarOffsets=offsets.data_ptr())
        args = (calls[0].inputs, a.num_reads, some, scratches[0].address)
        g.alignment_strings(calls[0].inputs, 0, None, 0)  # no reads: succeeds, touches nothing
        g.alignment_strings(calls[0].inputs, a.num_reads, awfm.string_outputs(), scratches[0].address, max_candidates=4)  # every output NULL
        for kw in (dict(max_candidates=0), dict(max_candidates=17), dict(max_ops=0), dict(max_ops=sc.MAX_OPS + 1), dict(flags=2), dict(flags=1 << 31)):
            with pytest.raises(awfm.AwFmError) as e:
                g.alignment_strings(*args, **dict(dict(max_candidates=4), **kw))
            assert e.value.rc == awfm.AwFmIllegalPositionError, kw
        with pytest.raises(awfm.AwFmError) as e:
            g.alignment_strings(calls[0].inputs, 1 << 32, some, scratches[0].address)
        assert e.value.rc == awfm.AwFmIllegalPositionError
        with pytest.raises(awfm.AwFmError) as e:  # a scratch that is not aligned to 16 bytes
            g.alignment_strings(*(args[:3] + (scratches[0].address + 8,)))
        assert e.value.rc == awfm.AwFmIllegalPositionError
        arena = torch.full((256,), PATTERN, dtype=torch.uint8, device="cuda")
        for bad in ((None,) + args[1:], args[:2] + (None,) + args[3:], args[:3] + (0,),
                    args[:2] + (awfm.string_outputs(cigarChars=arena.data_ptr(), cigarCapacity=256),) + args[3:],
                    args[:2] + (awfm.string_outputs(mdChars=arena.data_ptr(), mdCapacity=256, cigarOffsets=offsets.data_ptr()),) + args[3:],
                    (awfm.string_inputs(0, *(calls[0].buffers[name][1] for name in ("slots", "text_begins", "num_ops", "ops"))),) + args[1:],
                    (awfm.string_inputs(*(calls[0].buffers[name][1] for name in ("sequences", "slots", "text_begins", "num_ops")), 0),) + args[1:]):
            with pytest.raises(awfm.AwFmError) as e:
                g.alignment_strings(*bad)
            assert e.value.rc == sc.NULL_ERROR
        torch.cuda.synchronize()
        assert (offsets.cpu().numpy() == PATTERN).all() and (arena.cpu().numpy() == PATTERN).all()
        assert g.alignment_strings_scratch_bytes(0) == 0 and g.alignment_strings_scratch_bytes(1 << 32) == 0
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        pending = []
        for _ in range(3):  # a call's scratch is its own until it has finished: the calls of a stream follow each other
            for call, classic, s, scratch, w in zip(calls, (False, True), streams, scratches, want):
                pending.append(call.run(g, scratch, classic=classic, stream=s.cuda_stream, launch=False, want=w))
        for enqueue, _ in pending:  # interleaved, nothing waited for in between
            enqueue()
        torch.cuda.synchronize()
        for k, (_, collect) in enumerate(pending):
            got = collect()
            sc.assert_same(got, twins[k % 2], what=f"call {k}, twin")
            sc.assert_same(got, want[k % 2], what=f"call {k}, restatement")
        for s in streams:
            g.stream_retire(s.cuda_stream)
    finally:
        image.close()


def _text_interval_from(read, runs, md, table):
    """the text interval rebuilt from the read, the script and MD: '=' takes the read's letter, X and D take MD's letters; also
    checks MD's form and its count of matched positions"""
    import re
    assert re.fullmatch(rb"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*", md), md
    tokens = re.findall(rb"[0-9]+|\^[A-Z]+|[A-Z]", md)
    matched = sum(int(t) for t in tokens if t.isdigit()) + sum(1 for t in tokens if t.isalpha())
    assert matched == sum(n for n, op in runs if op in (sc.EQ, sc.X)), (md, runs)
    letters = iter(b"".join(t.lstrip(b"^") for t in tokens if not t.isdigit()))
    out, i = bytearray(), 0
    for n, op in runs:
        if op == sc.EQ:
            out += read[i:i + n].translate(table)
        elif op in (sc.X, sc.D):
            out += bytes(next(letters) for _ in range(n))
        i += n if op != sc.D else 0
    assert next(letters, None) is None and i == len(read)
    return bytes(out)


def _lengths_of(cigar):
    import re
    runs = [(int(n), op) for n, op in re.findall(rb"([0-9]+)([MIDS=X])", cigar)]
    assert b"".join(str(n).encode() + op for n, op in runs) == cigar
    return sum(n for n, op in runs if op in b"MIS=X"), sum(n for n, op in runs if op in b"MD=X")


def test_end_to_end_from_a_fasta_file(awfm, require_gpu, tmp_path):
    """reads -> longest suffix matches -> hit offsets -> locate -> local positions -> candidates -> chains -> verification ->
    affine alignment, and chain alignment, of verification's best slots -> the strings of both, on one stream, every call's arrays
    passed straight to the next.  The strings equal the host twin's and the restatement's; for every aligned read the text
    interval rebuilt from the read, the script and MD is letter(text[textBegin, textEnd)), MD counts the script's '=' and X
    positions, and the classic CIGAR has the extended one's read and text lengths."""
    import re
    import torch
    import align_chains_common as ac
    import read_candidates_common as rc
    import verify_chains_common as vc
    from test_gpu_verify_chains import _upload
    fa, records, reads, planted = ac.planted_inside(str(tmp_path), vc.E2E_W)
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "records.awfmi"))
    g = awfm.GpuIndex(ix)
    text, record_ends = vc.text_of(records)
    g.set_text(text)
    chars, starts, ends, offsets, seed_ends = rc.windows_of(reads)
    n, num_reads, slots, max_ops, L = len(starts), len(reads), 4, 32, rc.E2E_READ_LENGTH
    stream_obj = torch.cuda.Stream()
    s = stream_obj.cuda_stream
    d_chars, d_starts, d_ends, d_offsets, d_seed_ends = [_upload(torch, a) for a in (chars, starts, ends, offsets, seed_ends)]
    d_lengths, d_counts = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    d_ranges = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    d_hit_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_scan = torch.zeros(awfm.GpuIndex.scan_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g.longest_suffix_matches(d_chars.data_ptr(), d_starts.data_ptr(), d_ends.data_ptr(), 0, n, rc.E2E_MIN_LENGTH, d_lengths.data_ptr(),
                             d_ranges.data_ptr(), d_counts.data_ptr(), s)
    total = g.hit_offsets_from_counts(d_counts.data_ptr(), n, d_hit_offsets.data_ptr(), d_scan.data_ptr(), s)
    d_positions = torch.zeros(total, dtype=torch.int64, device="cuda")
    d_sequences = torch.zeros(total, dtype=torch.int32, device="cuda")
    slot32 = {name: torch.zeros(num_reads * slots, dtype=torch.int32, device="cuda") for name in ("sequences", "diagonalSpans", "chainAnchors", "chainReadBegins", "chainReadEnds", "votes")}
    slot64 = {name: torch.zeros(num_reads * slots, dtype=torch.int64, device="cuda") for name in ("diagonals", "chainBeginDiagonals", "chainEndDiagonals")}
    d_scratch = torch.zeros(max(awfm.read_candidates_scratch_bytes(num_reads), awfm.read_chains_scratch_bytes(num_reads)), dtype=torch.uint8, device="cuda")
    d_read_offsets = _upload(torch, np.arange(num_reads + 1, dtype=np.uint64) * L)
    d_best = torch.full((num_reads,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_trace = torch.zeros(max(g.align_chains_affine_scratch_bytes(L), g.align_chains_scratch_bytes(L)), dtype=torch.uint8, device="cuda")
    stream_obj.wait_stream(torch.cuda.current_stream())
    g.locate(d_ranges.data_ptr(), d_hit_offsets.data_ptr(), n, total, d_positions.data_ptr(), s)
    g.local_positions(d_positions.data_ptr(), total, d_sequences.data_ptr(), d_positions.data_ptr(), stream=s)
    inputs = awfm.candidate_inputs(d_offsets.data_ptr(), n, d_seed_ends.data_ptr(), d_lengths.data_ptr(), 0, d_hit_offsets.data_ptr(), total,
                                   d_positions.data_ptr(), d_sequences.data_ptr())
    cand = awfm.candidate_outputs(sequences=slot32["sequences"].data_ptr(), diagonals=slot64["diagonals"].data_ptr(),
                                  diagonalSpans=slot32["diagonalSpans"].data_ptr(), votes=slot32["votes"].data_ptr())
    g.read_candidates(inputs, num_reads, cand, d_scratch.data_ptr(), max_hits_per_seed=rc.E2E_MAX_HITS, band=2, min_votes=2, max_candidates=slots, stream=s)
    chain_names = ("chainAnchors", "chainReadBegins", "chainReadEnds", "chainBeginDiagonals", "chainEndDiagonals")
    chains = awfm.chain_outputs(**{name: (slot32.get(name) if name in slot32 else slot64[name]).data_ptr() for name in chain_names})
    g.read_chains(inputs, num_reads, slot32["sequences"].data_ptr(), slot64["diagonals"].data_ptr(), slot32["diagonalSpans"].data_ptr(), chains,
                  d_scratch.data_ptr(), max_hits_per_seed=rc.E2E_MAX_HITS, band=2, max_candidates=slots, gap_penalty=1, stream=s)
    vin = awfm.verify_inputs(d_chars.data_ptr(), len(chars), d_read_offsets.data_ptr(), sequences=slot32["sequences"].data_ptr(),
                             **{name: (slot32.get(name) if name in slot32 else slot64[name]).data_ptr() for name in chain_names})
    g.verify_chains(vin, num_reads, awfm.verify_outputs(bestSlots=d_best.data_ptr()), max_candidates=slots, band_pad=vc.E2E_W, max_drift=vc.E2E_X, stream=s)
    table, host_text = sc.letter_table(sc.DNA), text.tobytes()
    aligned = 0
    for affine in (True, False):
        d_begins = torch.zeros(num_reads, dtype=torch.int64, device="cuda")
        d_ends_text = torch.zeros(num_reads, dtype=torch.int64, device="cuda")
        d_num_ops = torch.zeros(num_reads, dtype=torch.int32, device="cuda")
        d_ops = torch.full((num_reads * max_ops,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        stream_obj.wait_stream(torch.cuda.current_stream())
        addresses = dict(textBegins=d_begins.data_ptr(), textEnds=d_ends_text.data_ptr(), numOps=d_num_ops.data_ptr(), ops=d_ops.data_ptr())
        if affine:
            g.align_chains_affine(vin, d_best.data_ptr(), num_reads, awfm.affine_outputs(**addresses), d_trace.data_ptr(), max_candidates=slots,
                                  band_pad=vc.E2E_W, max_drift=vc.E2E_X, max_ops=max_ops, max_rows=L, stream=s)
        else:
            g.align_chains(vin, d_best.data_ptr(), num_reads, awfm.align_outputs(**addresses), d_trace.data_ptr(), max_candidates=slots,
                           band_pad=vc.E2E_W, max_drift=vc.E2E_X, max_ops=max_ops, max_rows=L, stream=s)
        # the arrays go into the call as they lie on the device; capacities of 128 bytes a read hold every string here
        capacity = 128 * num_reads
        sin = awfm.string_inputs(slot32["sequences"].data_ptr(), d_best.data_ptr(), d_begins.data_ptr(), d_num_ops.data_ptr(), d_ops.data_ptr())
        scratch = Scratch(torch, g, num_reads)
        results = {}
        for classic in (False, True):
            out = {name: torch.full((size,), PATTERN, dtype=torch.uint8, device="cuda")
                   for name, size in (("cigarOffsets", 8 * (num_reads + 1)), ("cigarChars", capacity), ("mdOffsets", 8 * (num_reads + 1)), ("mdChars", capacity))}
            d_counters = torch.zeros(2, dtype=torch.int64, device="cuda")
            stream_obj.wait_stream(torch.cuda.current_stream())
            g.alignment_strings(sin, num_reads, awfm.string_outputs(cigarCapacity=capacity, mdCapacity=capacity, numSkipped=d_counters.data_ptr(),
                                                                     numOverflow=d_counters.data_ptr() + 8, **{k: v.data_ptr() for k, v in out.items()}),
                                scratch.address, max_candidates=slots, max_ops=max_ops, classic=classic, stream=s)
            stream_obj.synchronize()
            scratch.check()
            got = {k: v.cpu().numpy().view(np.uint64 if k.endswith("Offsets") else np.uint8) for k, v in out.items()}
            got["numSkipped"], got["numOverflow"] = (int(v) for v in d_counters.cpu().numpy())
            results[classic] = got
            arrays = dict(sequences=slot32["sequences"].cpu().numpy().view(np.uint32).reshape(num_reads, slots), slots=d_best.cpu().numpy().view(np.uint32),
                          text_begins=d_begins.cpu().numpy().view(np.uint64), num_ops=d_num_ops.cpu().numpy().view(np.uint32),
                          ops=d_ops.cpu().numpy().view(np.uint32).reshape(num_reads, max_ops))
            twin = awfm.alignment_strings_host(text=text, sequence_ends=record_ends, classic=classic, cigar_capacity=capacity, md_capacity=capacity,
                                               fill=PATTERN, **arrays)
            sc.assert_same(got, twin, what=("end to end", affine, classic))
            assert got["numSkipped"] == 0 and got["numOverflow"] == 0
        extended = awfm.strings_of(results[False]["cigarOffsets"], results[False]["cigarChars"])
        classic_cigars = awfm.strings_of(results[True]["cigarOffsets"], results[True]["cigarChars"])
        mds = awfm.strings_of(results[False]["mdOffsets"], results[False]["mdChars"])
        assert mds == awfm.strings_of(results[True]["mdOffsets"], results[True]["mdChars"])
        case = sc.Case([], text, record_ends)
        for r in range(num_reads):
            k = int(arrays["num_ops"][r])
            if k == 0:
                assert extended[r] == classic_cigars[r] == mds[r] == b""
                continue
            aligned += 1
            runs = [(int(v) >> 4, int(v) & 15) for v in arrays["ops"][r, :k]]
            assert extended[r] == awfm.cigar_of(arrays["ops"][r, :k]).encode()
            begin = case.record_bounds(int(arrays["sequences"][r, int(arrays["slots"][r])]))[0] + int(arrays["text_begins"][r])
            length = sum(nn for nn, op in runs if op in (sc.EQ, sc.X, sc.D))
            assert length == int(d_ends_text[r].item()) - int(arrays["text_begins"][r])
            read = chars.tobytes()[r * L:(r + 1) * L]
            clipped = read[runs[0][0] if runs[0][1] == sc.S else 0:len(read) - (runs[-1][0] if runs[-1][1] == sc.S and len(runs) > 1 else 0)]
            inner = [(nn, op) for nn, op in runs if op != sc.S]
            assert _text_interval_from(clipped, inner, mds[r], table) == host_text[begin:begin + length].translate(table), (r, extended[r], mds[r])
            assert _lengths_of(classic_cigars[r]) == _lengths_of(extended[r]) == (L, length)
            assert b"=" not in classic_cigars[r] and b"X" not in classic_cigars[r] and not re.search(rb"M[0-9]+M", classic_cigars[r])
    assert aligned >= 2 * sum(p is not None for p in planted)
    g.stream_retire(s)
    g.destroy()
    ix.dealloc()
