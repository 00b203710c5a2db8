"""awfmTextWindows (include/awfm_gpu.h "chain verification", csrc/awfm_verify.c), the host twin and checker of
awfmGpuTextWindows: windows equal a NumPy slice with zero fill for every split of up to 4096 bytes, at the text's two ends, for
positions at and far beyond it, on texts of 1, 15, 16 and 17 bytes; and they equal what awFmReadSequenceFromFile reads from an
index written with storeOriginalSequence."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def windows_by_slices(text, positions, before, after):
    """the definition: text[p - before, p + after), zero outside [0, length)"""
    text = np.frombuffer(bytes(text), np.uint8)
    out = np.zeros((len(positions), before + after), np.uint8)
    for i, p in enumerate(int(p) for p in positions):
        if p >= len(text):
            continue
        lo, hi = max(p - before, 0), min(p + after, len(text))
        out[i, lo - (p - before):hi - (p - before)] = text[lo:hi]
    return out


def edge_positions(length):
    return np.array([0, length - 1, length, length + 1, 2 ** 63, 2 ** 64 - 1, length // 2, 1 % max(length, 1)], np.uint64)


@pytest.mark.parametrize("length", [1, 15, 16, 17, 5000])
def test_windows_equal_numpy_slices_with_zero_fill(awfm, length):
    rng = np.random.default_rng(length)
    text = rng.integers(1, 256, length, dtype=np.uint8)
    positions = np.concatenate((edge_positions(length), rng.integers(0, length + 3, 40).astype(np.uint64)))
    for before, after in ((0, 1), (1, 0), (3, 4), (32, 32), (0, 4096), (4096, 0), (2048, 2048), (17, 1000), (4095, 1)):
        got = awfm.text_windows_host(text, positions, before, after, threads=3)
        assert np.array_equal(got, windows_by_slices(text, positions, before, after)), (before, after)


def test_widths_outside_1_to_4096_are_refused_and_no_positions_touch_nothing(awfm):
    text = np.arange(1, 50, dtype=np.uint8)
    for before, after in ((0, 0), (4096, 1), (1, 4096), (2 ** 32 - 1, 2)):
        with pytest.raises(awfm.AwFmError) as e:
            awfm.text_windows_host(text, [3], before, after)
        assert e.value.rc == awfm.AwFmIllegalPositionError
    assert awfm.text_windows_host(text, [], 3, 3).shape == (0, 6)
    assert awfm._lib.lib().awfmTextWindows(None, 0, None, 0, 1, 1, None, 1) == awfm.AwFmSuccess


def test_windows_equal_the_stored_sequence_of_an_index_file(awfm, tmp_path):
    """an index written with storeOriginalSequence keeps the text for awFmReadSequenceFromFile (one segment per call): the batched
    recall of the same text gives the same bytes wherever the segment lies inside the text"""
    rng = np.random.default_rng(4)
    text = rng.choice(np.frombuffer(b"acgt", np.uint8), 700)
    ix = awfm.create_index(text, awfm.AwFmAlphabetDna, 4, 4, store_sequence=True, file_src=str(tmp_path / "stored.awfmi"))
    try:
        positions = np.concatenate(([40, 659, 350], rng.integers(40, 660, 30))).astype(np.uint64)
        got = awfm.text_windows_host(text, positions, 40, 40)
        lib = awfm._lib.lib()
        for i, p in enumerate(int(p) for p in positions):
            buffer = C.create_string_buffer(81)
            rc = lib.awFmReadSequenceFromFile(ix.c, p - 40, 80, buffer)
            assert rc in (awfm.AwFmSuccess, awfm.AwFmFileReadOkay), rc
            assert bytes(got[i]) == buffer.raw[:80], p
    finally:
        ix.dealloc()
