"""The kept hits of a read are defined once for awfmGpuReadCandidates and awfmGpuReadChains (csrc/awfm_hits_kernel.h): both
device calls on the table of tests/test_kept_hits.py -- the edge list (0, 1, 4096 and 4097 kept hits), every malformed shape and
dropped seeds of 63, 64 and 65 hits and more, at maxHitsPerSeed 0, 1 and 3, the chains on the candidates' own slots -- by
default and with the workgroup tier forced report the same keptHits as each other and as the host twins, add the same number to
numOverflowed, and refuse the same arguments with the same code and with the texts the launchers had before they shared them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kept_hits_common as kh  # noqa: E402
import read_candidates_common as rc  # noqa: E402
from test_gpu_read_candidates import DeviceCall as CandidatesCall  # noqa: E402
from test_gpu_read_chains import DeviceCall as ChainsCall  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def image(awfm, require_gpu):
    """the calls read nothing of the index: any small image serves"""
    ix = awfm.create_index(np.frombuffer(b"acgtacgtacgtacgt" * 8, np.uint8), awfm.AwFmAlphabetDna, 2, 2)
    g = awfm.GpuIndex(ix)
    yield g
    g.destroy()
    ix.dealloc()


@pytest.fixture(scope="module")
def table(awfm):
    return kh.host_table(awfm)


@pytest.mark.parametrize("tier", [None, "group"], ids=["default", "group"])
def test_both_units_report_the_kept_hits_of_the_twins(awfm, image, diag, table, tier):
    import torch
    diag(candidates_tier=tier, chains_tier=tier)
    uploaded = {}
    for what, inst, m, case, candidates, chains in table:
        assert np.array_equal(candidates["keptHits"], chains["keptHits"]) and candidates["numOverflowed"] == chains["numOverflowed"], what
        call = uploaded.setdefault(id(inst), CandidatesCall(awfm, torch, inst))
        got = call(image, overflowed_before=kh.OVERFLOWED_BEFORE, max_candidates=kh.SLOTS, max_hits_per_seed=m, band=kh.BAND)
        got_chains = ChainsCall(awfm, torch, case)(image, overflowed_before=kh.OVERFLOWED_BEFORE, max_hits_per_seed=m, band=kh.BAND)
        for unit, result in (("candidates", got), ("chains", got_chains)):
            assert np.array_equal(result["keptHits"], candidates["keptHits"]), (what, unit, result["keptHits"].tolist())
            assert result["numOverflowed"] == candidates["numOverflowed"], (what, unit, result["numOverflowed"])


class Arguments:
    """a good call of either unit on four reads: device arrays, slot arrays, scratch"""

    def __init__(self, awfm, torch):
        self.inst = rc.random_instance(5, reads=4)
        self.call = CandidatesCall(awfm, torch, self.inst)
        self.slots = [torch.zeros(4 * 17 * 8, dtype=torch.uint8, device="cuda") for _ in range(3)]
        self.scratch = torch.zeros(max(awfm.read_candidates_scratch_bytes(4), awfm.read_chains_scratch_bytes(4)), dtype=torch.uint8, device="cuda")
        self.candidate_out, self.chain_out = awfm.candidate_outputs(), awfm.chain_outputs()

    def both(self, L, handle, inputs, num_reads, slots, with_outputs=True, scratch=True, slot_arrays=(True, True, True), lookback=64):
        """-> [(the call's name, its code, the library's last error text)] of the two device calls"""
        d_scratch = self.scratch.data_ptr() if scratch else None
        d_slots = [a.data_ptr() if given else None for a, given in zip(self.slots, slot_arrays)]
        out = []
        code = L.awfmGpuReadCandidates(handle, kh.byref_or_null(inputs), num_reads, 0, kh.BAND, 1, slots,
                                       kh.byref_or_null(self.candidate_out if with_outputs else None), d_scratch, None)
        out.append(("awfmGpuReadCandidates", code, L.awfmGpuLastError().decode()))
        code = L.awfmGpuReadChains(handle, kh.byref_or_null(inputs), num_reads, 0, kh.BAND, slots, *d_slots, lookback, 0,
                                   kh.byref_or_null(self.chain_out if with_outputs else None), d_scratch, None)
        out.append(("awfmGpuReadChains", code, L.awfmGpuLastError().decode()))
        return out


@pytest.fixture(scope="module")
def arguments(awfm, image):
    import torch
    return Arguments(awfm, torch)


@pytest.mark.parametrize("what,changes,code,text", kh.REFUSALS, ids=[r[0] for r in kh.REFUSALS])
def test_both_units_refuse_the_same_arguments_with_their_texts(awfm, image, arguments, what, changes, code, text):
    import torch
    from avxwindowfmindex_amd import _lib
    inputs, num_reads, slots, with_outputs = kh.refused_call(awfm, arguments.call.inputs, 4, changes)
    for name, got, message in arguments.both(_lib.lib(), image.handle, inputs, num_reads, slots, with_outputs):
        assert got == code, (what, name, got)
        assert text is None or message == f"{name}: {text}", (what, name, message)
    torch.cuda.synchronize()


def test_what_only_the_device_calls_refuse(awfm, image, arguments):
    """no image, no scratch; the chains' own: a missing slot array, a lookback outside 1 .. 64 (behind the shared refusals)"""
    import torch
    from avxwindowfmindex_amd import _lib
    L, inputs = _lib.lib(), arguments.call.inputs
    for name, got, message in arguments.both(L, None, inputs, 4, kh.SLOTS):
        assert got == kh.NULL_PTR and message == f"{name}: null image", (name, got, message)
    for name, got, message in arguments.both(L, image.handle, inputs, 4, kh.SLOTS, scratch=False):
        assert got == kh.NULL_PTR and message == f"{name}: null argument", (name, got, message)
    for missing in range(3):
        results = arguments.both(L, image.handle, inputs, 4, kh.SLOTS, slot_arrays=[k != missing for k in range(3)])
        assert results[0][1] == kh.SUCCESS and results[1][1:] == (kh.NULL_PTR, "awfmGpuReadChains: null argument"), results
    for lookback in (0, 65):
        results = arguments.both(L, image.handle, inputs, 4, kh.SLOTS, lookback=lookback)
        assert results[0][1] == kh.SUCCESS, results
        assert results[1][1:] == (kh.ILLEGAL, "awfmGpuReadChains: an anchor looks back at 1 to 64 anchors"), results
    results = arguments.both(L, image.handle, inputs, 4, 17, lookback=0)  # the shared refusals come first
    assert results[1][1:] == (kh.ILLEGAL, "awfmGpuReadChains: " + kh.RANGE_TEXT), results
    torch.cuda.synchronize()
