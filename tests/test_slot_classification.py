"""The classification of a chain slot -- unused, malformed, too wide, or "has a band" -- is one definition (csrc/awfm_band.h on the
host, csrc/awfm_band_kernel.h on the device) used by chain verification, chain alignment, affine alignment and slot scoring.
One table of slot shapes, every shape alone and combined with the one after it so that the order of the checks shows, goes
through the four host calls: they agree on the class of every slot, and the classes equal a literal list recorded from the
library as it was when each of the four files still carried its own copy of the checks.  On the device the same table goes
through the four device calls at the natural number of lanes and with 64 forced, and every output equals the host twin's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import align_chains_common as ac  # noqa: E402
import score_chains_common as sc  # noqa: E402
import verify_chains_common as vc  # noqa: E402

C, W, X = 4, 2, 3  # slots per read, bandPad, maxDrift
CLASS = {vc.NONE: "N", vc.MALFORMED: "M", vc.TOO_WIDE: "W"}  # anything else: "B", the slot has a band
RECORDS = [bytes(np.random.default_rng(7).choice(np.frombuffer(b"acgt", np.uint8), n)) for n in (40, 30, 50)]
READ = RECORDS[1][5:17]  # twelve characters of record 1 on diagonal 5
#: the good slot: characters 2 .. 10 of the read against 7 .. 15 of record 1 (30 characters long)
GOOD = dict(s=1, anchors=1, rb=2, re=10, bD=5, eD=5, reversed=False, ends=None)
BIG = 2 ** 64 - 1


def _ends(spec, k, value, s):
    ends = list(spec["ends"])
    ends[k] = value
    return dict(spec, ends=ends, s=s)


#: (name, what the shape does to a slot).  A read-level shape (the offsets) and the shapes of the ends table hold for the whole read
SHAPES = [
    ("unused sequence", lambda p: dict(p, s=vc.NONE)),
    ("zero anchors", lambda p: dict(p, anchors=0)),
    ("read offsets reversed", lambda p: dict(p, reversed=True)),
    ("rb > re", lambda p: dict(p, rb=p["re"] + 1)),
    ("re beyond the read", lambda p: dict(p, re=len(READ) + 1)),
    ("record number equal to numRecords", lambda p: dict(p, s=len(RECORDS))),
    ("a record end of 2^64 - 1 before it", lambda p: _ends(p, 1, BIG, 2)),
    ("E beyond the text", lambda p: _ends(p, 2, 200, 2)),
    ("bD = 2^62", lambda p: dict(p, bD=2 ** 62)),
    ("eD = -2^62", lambda p: dict(p, eD=-2 ** 62)),
    ("bD = 2^63 - 1", lambda p: dict(p, bD=2 ** 63 - 1)),
    ("eD = -(2^63 - 1)", lambda p: dict(p, eD=-(2 ** 63 - 1))),
    ("bD = -2^33 - 1", lambda p: dict(p, bD=-2 ** 33 - 1)),
    ("eD = -2^33 + 1", lambda p: dict(p, eD=-2 ** 33 + 1)),
    ("eD = 2^62", lambda p: dict(p, eD=2 ** 62)),
    ("bD = -2^62", lambda p: dict(p, bD=-2 ** 62)),
    ("eD = 2^63 - 1", lambda p: dict(p, eD=2 ** 63 - 1)),
    ("bD = -(2^63 - 1)", lambda p: dict(p, bD=-(2 ** 63 - 1))),
    ("eD = -2^33 - 1", lambda p: dict(p, eD=-2 ** 33 - 1)),
    ("bD = -2^33 + 1", lambda p: dict(p, bD=-2 ** 33 + 1)),
    ("tb < 0", lambda p: dict(p, bD=-p["rb"] - 1, eD=-p["rb"] - 1)),
    ("te one beyond L", lambda p: dict(p, bD=len(RECORDS[1]) + 1 - p["re"], eD=len(RECORDS[1]) + 1 - p["re"])),
    ("drift equal to maxDrift", lambda p: dict(p, eD=p["bD"] + X)),
    ("drift one more", lambda p: dict(p, eD=p["bD"] + X + 1)),
]

#: per read the classes of its four slots: the shaped slot is slot r mod 4, the good slot follows it, the other two are unused.
#: Read 2 k is shape k alone, read 2 k + 1 is shape k with shape k + 1 applied on top of it.  Recorded from the four separate
#: copies of the checks (the commit before the shared definition), which agreed on every slot
EXPECTED = ["NBNN", "NNBN", "NNNB", "MNNN", "MMNN", "NMMN", "NNMB", "BNNM", "MBNN", "NMBN", "NNMB", "MNNM", "MMNN", "NMMN", "NNMB", "BNNM",
            "MBNN", "NMBN", "NNMB", "BNNM", "MBNN", "NMBN", "NNMB", "BNNM", "MBNN", "NMBN", "NNMB", "BNNM", "MBNN", "NMBN", "NNMB", "BNNM",
            "MBNN", "NMBN", "NNMB", "BNNM", "MBNN", "NMBN", "NNMB", "BNNM", "MBNN", "NMBN", "NNMB", "BNNM", "BBNN", "NWBN", "NNWB"]


def table():
    """-> [(name, spec)] in the order of EXPECTED"""
    base = vc.Builder(RECORDS)
    good = dict(GOOD, ends=list(base.ends))
    rows = []
    for k, (name, shape) in enumerate(SHAPES):
        rows.append((name, shape(good)))
        if k + 1 < len(SHAPES):
            rows.append((name + " + " + SHAPES[k + 1][0], SHAPES[k + 1][1](shape(good))))
    return bytes(base.text), good, rows


def cases():
    """the table as calls: the reads that share an ends table make one -> [(read numbers in the table, sc.Case)]"""
    text, good, rows = table()
    by_ends = {}
    for r, (_, spec) in enumerate(rows):
        by_ends.setdefault(tuple(spec["ends"]), []).append(r)
    out = []
    for ends, reads in by_ends.items():
        slots = {name: np.zeros((2 * len(reads), C), vc.SLOT_DTYPES[name]) for name in vc.SLOT_FIELDS}
        slots["sequences"][:] = vc.NONE
        offsets, chosen = [], []
        for i, r in enumerate(reads):  # read 2 i of the call is the table's read r; read 2 i + 1 joins its end to the next one's begin
            spec, begin = rows[r][1], i * len(READ)
            offsets += [begin + len(READ), begin] if spec["reversed"] else [begin, begin + len(READ)]
            for j, p in ((r % C, spec), ((r + 1) % C, dict(good, ends=spec["ends"]))):
                for name, key in zip(vc.SLOT_FIELDS, ("s", "anchors", "rb", "re", "bD", "eD")):
                    slots[name][2 * i, j] = p[key]
            chosen += [r % C, 0]
        offsets.append(offsets[-1])
        out.append((reads, sc.Case(READ * len(reads), offsets, slots, chosen, text, np.array(ends, np.uint64))))
    return out


def classes(values):
    return "".join(CLASS.get(int(v), "B") for v in values)


def test_the_four_host_calls_agree_on_every_slot_and_equal_the_recorded_classes(awfm):
    _, _, rows = table()
    got = [None] * len(rows)
    for reads, case in cases():
        verified = vc.Case.host(case, awfm, W, X)["editDistances"]
        scored = case.score(awfm, W, X)["slotScores"]
        aligned, affine = np.zeros_like(verified), np.zeros_like(verified)
        kept = case.chosen
        for j in range(C):  # the two calls that take one slot a read, slot by slot
            case.chosen = np.full(case.num_reads, j, np.uint32)
            aligned[:, j] = ac.Case.host(case, awfm, W, X)["editDistances"]
            affine[:, j] = af.Case.host(case, awfm, W, X)["scores"]
        case.chosen = kept
        assert (verified[1::2] == vc.NONE).all()  # the reads in between have no slot
        for i, r in enumerate(reads):
            four = [classes(values[2 * i]) for values in (verified, aligned, affine, scored)]
            assert len(set(four)) == 1, (rows[r][0], four)
            got[r] = four[0]
    assert len(EXPECTED) == len(rows) == 2 * len(SHAPES) - 1
    assert got == EXPECTED, [(rows[r][0], g, w) for r, (g, w) in enumerate(zip(got, EXPECTED)) if g != w]
    # the table meets every class, and both drifts on either side of the bound
    assert {c for word in EXPECTED for c in word} == set("NMWB")
    assert EXPECTED[2 * 22][22 * 2 % C] == "B" and EXPECTED[2 * 23][23 * 2 % C] == "W"


@pytest.mark.gpu
@pytest.mark.parametrize("group", [None, 64], ids=["natural", "64"])
def test_the_four_device_calls_equal_their_twins_on_the_table(awfm, require_gpu, diag, group):
    import torch
    import test_gpu_align_affine as gaf
    import test_gpu_align_chains as gac
    import test_gpu_score_chains as gsc
    import test_gpu_verify_chains as gvc
    diag(verify_group=group, align_group=group, affine_group=group, score_group=group)
    ran = 0
    for reads, case in cases():
        if int(case.ends.max()) >= 2 ** 62:
            # the device never meets an end of 2^64 - 1: its record table refuses ends of 2^62 or more (the device's
            # classification relies on that), so these reads are the host's alone
            ix = awfm.create_index(case.text, awfm.AwFmAlphabetDna, 2, 2)
            g = awfm.GpuIndex(ix)
            try:
                with pytest.raises(awfm.AwFmError) as e:
                    g.set_record_table(case.ends)
                assert e.value.rc == awfm.AwFmIllegalPositionError
            finally:
                g.destroy()
                ix.dealloc()
            continue
        image = gvc.Image(awfm, case)
        try:
            vc.assert_equal(gvc.DeviceCall(awfm, torch, case)(image.g, W, X), vc.Case.host(case, awfm, W, X))
            sc.assert_equal(gsc.DeviceCall(awfm, torch, case)(image.g, W, X), case.score(awfm, W, X))
            scratch = gac.Scratch(torch, image.g, len(READ))
            ac.assert_equal(gac.DeviceCall(awfm, torch, case)(image.g, W, X, scratch), ac.Case.host(case, awfm, W, X))
            scratch = gaf.Scratch(torch, image.g, len(READ))
            af.assert_equal(gaf.DeviceCall(awfm, torch, case)(image.g, W, X, scratch), af.Case.host(case, awfm, W, X))
            ran += len(reads)
        finally:
            image.close()
    assert ran >= 2 * len(SHAPES) - 1 - 3  # all but the reads whose table holds 2^64 - 1
