"""awfmGpuIndexSetText / awfmGpuTextWindows (include/awfm_gpu.h "chain verification", csrc/awfm_verify_kernel.h) against the host
twin awfmTextWindows, which tests/test_text_windows.py pins to NumPy slices and to awFmReadSequenceFromFile: bit for bit, at
every alignment of window, width and output, with the count read from the device; the text's place in the image (bytes,
description, replacement, removal); the output lies between guard words."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_text_windows import edge_positions  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 64, 0xA5


def make_image(awfm, text):
    ix = awfm.create_index(np.ascontiguousarray(text, np.uint8), awfm.AwFmAlphabetDna, 2, 2)
    return ix, awfm.GpuIndex(ix)


def device_windows(awfm, torch, g, positions, before, after, count=None, skew=0):
    """the device call on an output that begins `skew` bytes into an aligned buffer, between guard words -> (windows, untouched
    rows past the count)"""
    positions = np.ascontiguousarray(positions, np.uint64)
    width, capacity = before + after, len(positions)
    d_positions = torch.from_numpy(positions.view(np.int64).copy()).to("cuda")
    out = torch.full((GUARD + skew + capacity * width + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    d_count = torch.tensor([capacity if count is None else count], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g.text_windows(d_positions.data_ptr(), capacity, before, after, out.data_ptr() + GUARD + skew, d_num_positions=0 if count is None else d_count.data_ptr())
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[:GUARD + skew] == PATTERN).all() and (raw[GUARD + skew + capacity * width:] == PATTERN).all(), "wrote outside the windows"
    return raw[GUARD + skew:GUARD + skew + capacity * width].reshape(capacity, width)


@pytest.mark.parametrize("length", [1, 15, 16, 17, 4099])
def test_windows_equal_the_host_twin_at_every_alignment(awfm, require_gpu, length):
    import torch
    rng = np.random.default_rng(length)
    text = rng.choice(np.frombuffer(b"acgtn", np.uint8), length)
    ix, g = make_image(awfm, text)
    try:
        assert g.text_length == 0
        g.set_text(text)
        assert g.text_length == length
        positions = np.concatenate((edge_positions(length), np.arange(min(length, 9), dtype=np.uint64), rng.integers(0, length + 3, 40).astype(np.uint64)))
        for k, (before, after) in enumerate(((0, 1), (1, 0), (3, 4), (2, 3), (32, 32), (0, 4096), (4096, 0), (2048, 2048), (17, 1000), (4095, 1), (33, 30))):
            want = awfm.text_windows_host(text, positions, before, after)
            got = device_windows(awfm, torch, g, positions, before, after, skew=k % 4)
            assert np.array_equal(got, want), (before, after, np.argwhere(got != want)[:4].tolist())
    finally:
        g.destroy()
        ix.dealloc()


def test_random_positions_with_the_count_read_from_the_device(awfm, require_gpu):
    import torch
    rng = np.random.default_rng(2)
    text = rng.choice(np.frombuffer(b"acgt", np.uint8), 1 << 16)
    ix, g = make_image(awfm, text)
    try:
        g.set_text(text)
        positions = rng.integers(0, (1 << 16) + 40, 1 << 16).astype(np.uint64)
        count = (1 << 16) - 4321
        for before, after, skew in ((32, 32, 0), (17, 46, 1), (1, 2, 3)):
            got = device_windows(awfm, torch, g, positions, before, after, count=count, skew=skew)
            assert np.array_equal(got[:count], awfm.text_windows_host(text, positions[:count], before, after, threads=8))
            assert (got[count:] == PATTERN).all(), "windows past the count were written"
    finally:
        g.destroy()
        ix.dealloc()


def test_the_text_belongs_to_the_image(awfm, require_gpu):
    """counted in the device bytes, named in the description, shared by the handles, replaced between two calls, removed; a text
    of another length is refused and leaves the old one; without a text the call is refused and writes nothing"""
    import torch
    rng = np.random.default_rng(3)
    text = rng.choice(np.frombuffer(b"acgt", np.uint8), 1000)
    ix, g = make_image(awfm, text)
    try:
        positions = np.arange(0, 1000, 7, dtype=np.uint64)
        d_positions = torch.from_numpy(positions.view(np.int64).copy()).to("cuda")
        out = torch.full((len(positions) * 8,), PATTERN, dtype=torch.uint8, device="cuda")
        with pytest.raises(awfm.AwFmError) as e:
            g.text_windows(d_positions.data_ptr(), len(positions), 4, 4, out.data_ptr())
        assert e.value.rc == awfm.AwFmUnsupportedVersionError
        torch.cuda.synchronize()
        assert (out == PATTERN).all()
        before_bytes = g.device_bytes
        assert "text:" not in g.describe()
        g.set_text(text)
        assert g.device_bytes == before_bytes + (1000 + 15) // 16 * 16 + 16
        assert "text: 1000 positions" in g.describe()
        for bad in (text[:-1], np.concatenate((text, text[:1]))):
            with pytest.raises(awfm.AwFmError) as e:
                g.set_text(bad)
            assert e.value.rc == awfm.AwFmIllegalPositionError and g.text_length == 1000
        with pytest.raises(awfm.AwFmError) as e:
            g.text_windows(d_positions.data_ptr(), len(positions), 0, 4097, out.data_ptr())
        assert e.value.rc == awfm.AwFmIllegalPositionError
        first = device_windows(awfm, torch, g, positions, 5, 6)
        other = text[::-1].copy()
        g.set_text(other)  # replaced between two calls
        second = device_windows(awfm, torch, g, positions, 5, 6)
        assert np.array_equal(first, awfm.text_windows_host(text, positions, 5, 6))
        assert np.array_equal(second, awfm.text_windows_host(other, positions, 5, 6))
        g.set_text(None)
        assert g.text_length == 0 and g.device_bytes == before_bytes
    finally:
        g.destroy()
        ix.dealloc()
