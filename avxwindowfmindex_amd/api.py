"""Python mirror of the AwFmIndex.h interface, calling libawfmindex_amd.so through its C ABI.

Names and argument meaning follow the reference API (src/AwFmIndex.h) so tests read
like the reference's own: create_index -> awFmCreateIndex, KmerSearchList ->
awFmCreateKmerSearchList, parallel_search_count / parallel_search_locate ->
awFmParallelSearchCount / awFmParallelSearchLocate.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import (AwFmAlphabetAmino, AwFmAlphabetDna, AwFmAlphabetRna, AwFmFileReadOkay, AwFmFileWriteOkay,  # noqa: F401
                   AwFmIllegalPositionError, AwFmSuccess, AwFmUnsupportedVersionError)

ILLEGAL_SEQUENCE = 0xFFFFFFFF  # the sequence number of an illegal position in the batch mappings (include/awfm_gpu.h)


class AwFmError(RuntimeError):
    def __init__(self, what, rc):
        msg = _lib.lib().awfmGpuLastError().decode(errors="replace")
        super().__init__(f"{what} failed with AwFmReturnCode {rc}" + (f": {msg}" if msg else ""))
        self.rc = rc


def _check(what, rc, ok=(AwFmSuccess, AwFmFileReadOkay, AwFmFileWriteOkay)):
    if rc not in ok:
        raise AwFmError(what, rc)
    return rc


class Index:
    """struct AwFmIndex* owner"""

    def __init__(self, ptr):
        self.ptr = ptr

    @property
    def c(self):
        return self.ptr.contents

    @property
    def bwt_length(self):
        return int(self.c.bwtLength)

    @property
    def sa_width(self):
        """bits per sampled suffix-array value (ref src/AwFmSuffixArray.c:12-18)"""
        return int(self.c.suffixArray.valueBitWidth)

    @property
    def is_amino(self):
        return self.c.config.alphabetType == AwFmAlphabetAmino

    @property
    def num_blocks(self):
        return 1 + (self.bwt_length - 1) // 256

    # host arrays in reference layout (views, valid while the index lives)
    def blocks(self):
        nbytes = self.num_blocks * (352 if self.is_amino else 160)
        return np.ctypeslib.as_array(C.cast(self.c.bwtBlockList, C.POINTER(C.c_uint8)), shape=(nbytes,))

    def prefix_sums(self):
        return np.ctypeslib.as_array(self.c.prefixSums, shape=((20 if self.is_amino else 4) + 2,))

    def seed_table(self):
        n = (20 if self.is_amino else 4) ** int(self.c.config.kmerLengthInSeedTable)
        return np.ctypeslib.as_array(C.cast(self.c.kmerSeedTable, C.POINTER(C.c_uint64)), shape=(n, 2))

    def packed_sa(self):
        sa = self.c.suffixArray
        if not sa.values:
            return None
        return np.ctypeslib.as_array(sa.values, shape=(int(sa.compressedByteLength),))

    def find_search_range_for_string(self, kmer):
        r = _lib.lib().awFmFindSearchRangeForString(self.ptr, bytes(kmer), len(kmer))
        return int(r.startPtr), int(r.endPtr)

    def local_position(self, global_position):
        """awFmGetLocalSequencePositionFromIndexPosition -> (sequence number, position in it)"""
        seq, loc = C.c_size_t(0), C.c_size_t(0)
        rc = _lib.lib().awFmGetLocalSequencePositionFromIndexPosition(self.ptr, global_position, C.byref(seq), C.byref(loc))
        _check("awFmGetLocalSequencePositionFromIndexPosition", rc)
        return int(seq.value), int(loc.value)

    def header(self, sequence_number):
        """awFmGetHeaderStringFromSequenceNumber"""
        buf, n = C.c_char_p(), C.c_size_t(0)
        rc = _lib.lib().awFmGetHeaderStringFromSequenceNumber(self.ptr, sequence_number, C.byref(buf), C.byref(n))
        _check("awFmGetHeaderStringFromSequenceNumber", rc)
        return C.string_at(buf, n.value)

    def dealloc(self):
        if self.ptr:
            _lib.lib().awFmDeallocIndex(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.dealloc()
        except Exception:
            pass


def create_index(sequence, alphabet=AwFmAlphabetDna, sa_ratio=8, seed_k=8, keep_sa_in_memory=True,
                 store_sequence=False, file_src=None):
    """awFmCreateIndex (ref src/AwFmIndex.h:164-169)"""
    L = _lib.lib()
    cfg = _lib.AwFmIndexConfiguration(sa_ratio, seed_k, alphabet, keep_sa_in_memory, store_sequence)
    seq = np.frombuffer(bytes(sequence), dtype=np.uint8) if not isinstance(sequence, np.ndarray) else sequence
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    holder = seq if seq.size else np.zeros(1, np.uint8)
    if file_src is None:
        file_src = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"awfm_{os.getpid()}_{id(seq):x}.awfmi")
    out = C.POINTER(_lib.AwFmIndex)()
    rc = L.awFmCreateIndex(C.byref(out), C.byref(cfg), holder.ctypes.data, seq.size, file_src.encode())
    _check("awFmCreateIndex", rc, ok=(AwFmFileWriteOkay,))
    ix = Index(out)
    ix.file_src = file_src
    return ix


def gpu_create_index(sequence, alphabet=AwFmAlphabetDna, sa_ratio=8, seed_k=8, keep_sa_in_memory=True,
                     store_sequence=False, file_src=None, device=-1, on_device_length=None):
    """awfmGpuCreateIndex: same arrays as create_index, built on the GPU.  `sequence` is bytes / a numpy
    array, or a device address (int) together with on_device_length."""
    L = _lib.lib()
    cfg = _lib.AwFmIndexConfiguration(sa_ratio, seed_k, alphabet, keep_sa_in_memory, store_sequence)
    out = C.POINTER(_lib.AwFmIndex)()
    if on_device_length is not None:
        rc = L.awfmGpuCreateIndex(C.byref(out), C.byref(cfg), int(sequence), on_device_length, 1,
                                  file_src.encode() if file_src else None, device)
    else:
        seq = np.frombuffer(bytes(sequence), dtype=np.uint8) if not isinstance(sequence, np.ndarray) else sequence
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        holder = seq if seq.size else np.zeros(1, np.uint8)
        rc = L.awfmGpuCreateIndex(C.byref(out), C.byref(cfg), holder.ctypes.data, seq.size, 0,
                                  file_src.encode() if file_src else None, device)
    _check("awfmGpuCreateIndex", rc, ok=(AwFmFileWriteOkay,))
    ix = Index(out)
    ix.file_src = file_src
    return ix


def create_index_from_fasta(fasta_src, alphabet=AwFmAlphabetDna, sa_ratio=8, seed_k=8, keep_sa_in_memory=True,
                            store_sequence=False, file_src=None):
    """awFmCreateIndexFromFasta (ref src/AwFmIndex.h:196-200)"""
    cfg = _lib.AwFmIndexConfiguration(sa_ratio, seed_k, alphabet, keep_sa_in_memory, store_sequence)
    if file_src is None:
        file_src = fasta_src + ".awfmi"
    out = C.POINTER(_lib.AwFmIndex)()
    rc = _lib.lib().awFmCreateIndexFromFasta(C.byref(out), C.byref(cfg), fasta_src.encode(), file_src.encode())
    _check("awFmCreateIndexFromFasta", rc, ok=(AwFmFileWriteOkay,))
    ix = Index(out)
    ix.file_src = file_src
    return ix


def read_index_from_file(file_src, keep_sa_in_memory=True):
    """awFmReadIndexFromFile (ref src/AwFmIndex.h:260-262)"""
    out = C.POINTER(_lib.AwFmIndex)()
    rc = _lib.lib().awFmReadIndexFromFile(C.byref(out), file_src.encode(), keep_sa_in_memory)
    _check("awFmReadIndexFromFile", rc, ok=(AwFmFileReadOkay,))
    ix = Index(out)
    ix.file_src = file_src
    return ix


class KmerSearchList:
    """struct AwFmKmerSearchList* owner; fill() sets kmerString/kmerLength like the reference tests do"""

    def __init__(self, capacity):
        self.ptr = _lib.lib().awFmCreateKmerSearchList(capacity)
        if not self.ptr:
            raise MemoryError("awFmCreateKmerSearchList")
        self._keep = None

    def fill(self, kmers):
        lst = self.ptr.contents
        assert len(kmers) <= lst.capacity
        bufs = [C.create_string_buffer(bytes(k), len(k)) if len(k) else C.create_string_buffer(1) for k in kmers]
        for i, (k, b) in enumerate(zip(kmers, bufs)):
            lst.kmerSearchData[i].kmerString = C.addressof(b)
            lst.kmerSearchData[i].kmerLength = len(k)
        lst.count = len(kmers)
        self._keep = bufs

    def counts(self):
        lst = self.ptr.contents
        return np.array([lst.kmerSearchData[i].count for i in range(lst.count)], dtype=np.uint32)

    def capacities(self):
        lst = self.ptr.contents
        return np.array([lst.kmerSearchData[i].capacity for i in range(lst.count)], dtype=np.uint32)

    def positions(self, i):
        d = self.ptr.contents.kmerSearchData[i]
        if not d.count:
            return np.zeros(0, np.uint64)
        return np.ctypeslib.as_array(d.positionList, shape=(d.count,)).astype(np.uint64)

    def dealloc(self):
        if self.ptr:
            _lib.lib().awFmDeallocKmerSearchList(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.dealloc()
        except Exception:
            pass


def parallel_search_count(index, search_list, num_threads=4):
    """awFmParallelSearchCount (ref src/AwFmIndex.h:400-403); returns nothing, like the reference"""
    _lib.lib().awFmParallelSearchCount(index.ptr, search_list.ptr, num_threads)


def parallel_search_locate(index, search_list, num_threads=4):
    """awFmParallelSearchLocate (ref src/AwFmIndex.h:364-367); returns the AwFmReturnCode"""
    return _lib.lib().awFmParallelSearchLocate(index.ptr, search_list.ptr, num_threads)


def pack_kmers(kmers, alphabet=AwFmAlphabetDna):
    """awfmPackKmers: uint8[n, L] fixed-length ASCII k-mers -> uint64[n] packed words (2 bits per nucleotide, 5 bits
    per amino acid, first character most significant).  Raises on a k-mer the packing cannot express."""
    kmers = np.ascontiguousarray(kmers, dtype=np.uint8)
    n, length = kmers.shape
    out = np.zeros(n, np.uint64)
    bad = C.c_uint64(0)
    holder = kmers if kmers.size else np.zeros(1, np.uint8)
    rc = _lib.lib().awfmPackKmers(alphabet, holder.ctypes.data, length, n, out.ctypes.data, C.byref(bad))
    if rc != AwFmSuccess:
        raise ValueError(f"awfmPackKmers: k-mer {bad.value} cannot be packed (rc {rc})")
    return out


def local_positions_host(index, positions, threads=4, out_sequence=None, out_local=None):
    """awfmLocalPositions: global text positions (uint64[n]) -> (sequence numbers uint32[n], local positions uint64[n],
    how many are illegal); an illegal position gets ILLEGAL_SEQUENCE and keeps its global position.  out_local may be
    `positions` itself (in place).  Raises AwFmError (rc AwFmUnsupportedVersionError) on an index without a record table."""
    positions = np.ascontiguousarray(positions, dtype=np.uint64)
    n = positions.size
    seq = np.zeros(n, np.uint32) if out_sequence is None else out_sequence
    local = np.zeros(n, np.uint64) if out_local is None else out_local
    assert seq.dtype == np.uint32 and local.dtype == np.uint64 and seq.size >= n and local.size >= n
    illegal = C.c_uint64(0)
    rc = _lib.lib().awfmLocalPositions(index.ptr, positions.ctypes.data if n else None, n, seq.ctypes.data if n else None,
                                       local.ctypes.data if n else None, C.byref(illegal), threads)
    _check("awfmLocalPositions", rc)
    return seq, local, int(illegal.value)


def longest_suffix_matches_host(index, chars, starts=None, ends=None, fixed_length=0, min_length=0, threads=4):
    """awfmLongestSuffixMatches: for query i = chars[starts[i]:ends[i]] (both None: fixed_length characters per query, chars
    then holds a whole number of them) the length of its longest suffix that occurs in the text, the BWT range of that suffix
    and its size -> (match lengths uint32[n], ranges uint64[n, 2], counts uint32[n]).  A query whose match is shorter than
    max(min_length, 1) gets the range (1, 0) and count 0; the length is the true one either way."""
    chars = np.ascontiguousarray(np.frombuffer(chars, np.uint8) if isinstance(chars, (bytes, bytearray)) else chars, dtype=np.uint8)
    if (starts is None) != (ends is None):
        raise ValueError("starts and ends come together")
    if starts is not None:
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        ends = np.ascontiguousarray(ends, dtype=np.uint64)
        if starts.shape != ends.shape:
            raise ValueError("starts and ends differ in length")
        n = starts.size
    else:
        if fixed_length <= 0:
            raise ValueError("queries need starts and ends or a fixed length")
        n = chars.size // fixed_length
    lengths = np.zeros(n, np.uint32)
    ranges = np.zeros((n, 2), np.uint64)
    counts = np.zeros(n, np.uint32)
    holder = chars if chars.size else np.zeros(1, np.uint8)
    rc = _lib.lib().awfmLongestSuffixMatches(index.ptr, holder.ctypes.data, starts.ctypes.data if starts is not None and n else None,
                                             ends.ctypes.data if ends is not None and n else None, fixed_length, n, min_length,
                                             lengths.ctypes.data if n else None, ranges.ctypes.data if n else None,
                                             counts.ctypes.data if n else None, threads)
    _check("awfmLongestSuffixMatches", rc)
    return lengths, ranges, counts


CANDIDATES_MAX_HITS = 4096  # AWFM_CANDIDATES_MAX_HITS: kept hits per read beyond which a read is overflowed (include/awfm_gpu.h)
CANDIDATES_NONE = 0xFFFFFFFF  # the sequence of an unused candidate slot
CANDIDATE_SLOT_OUTPUTS = (("sequences", np.uint32), ("diagonals", np.int64), ("votes", np.uint32), ("diagonalSpans", np.uint32),
                          ("readBegins", np.uint32), ("readEnds", np.uint32))
CANDIDATE_READ_OUTPUTS = (("numCandidates", np.uint32), ("keptHits", np.uint32))


def candidate_inputs(read_seed_offsets, num_seeds, seed_ends, seed_lengths, fixed_length, hit_offsets, num_hits, positions,
                     sequence_numbers):
    """struct AwFmCandidateInputs from addresses (ints; 0 or None: NULL), host or device alike"""
    return _lib.AwFmCandidateInputs(read_seed_offsets or None, num_seeds, seed_ends or None, seed_lengths or None, fixed_length,
                                    hit_offsets or None, num_hits, positions or None, sequence_numbers or None)


def candidate_outputs(**addresses):
    """struct AwFmCandidateOutputs from addresses by field name (sequences, diagonals, votes, diagonalSpans, readBegins, readEnds,
    numCandidates, keptHits, numOverflowed); a field left out is NULL"""
    out = _lib.AwFmCandidateOutputs()
    for name, address in addresses.items():
        if name not in dict(_lib.AwFmCandidateOutputs._fields_):
            raise ValueError(f"no output called {name}")
        setattr(out, name, address or None)
    return out


def read_candidates_host(read_seed_offsets, seed_ends, hit_offsets, positions, sequence_numbers=None, seed_lengths=None, fixed_length=0,
                         max_hits_per_seed=0, band=0, min_votes=1, max_candidates=4, threads=4, outputs=None, num_seeds=None,
                         num_hits=None, fill=None, overflowed_before=0):
    """awfmReadCandidates (include/awfm_gpu.h, "candidate loci"): the seeds [read_seed_offsets[r], read_seed_offsets[r + 1]) of
    read r, their hits [hit_offsets[s], hit_offsets[s + 1]) of positions / sequence_numbers -> a dict of the outputs by field
    name: the six per-slot arrays shaped (reads, max_candidates), numCandidates and keptHits per read, numOverflowed (an int:
    overflowed_before plus this call's).  outputs: the names to compute (None: all); the others are passed as NULL and left out.
    num_seeds / num_hits default to the arrays' sizes; fill: the value (per byte) the arrays hold before the call."""
    o = np.ascontiguousarray(read_seed_offsets, dtype=np.uint64)
    ends = np.ascontiguousarray(seed_ends, dtype=np.uint32)
    ho = np.ascontiguousarray(hit_offsets, dtype=np.uint64)
    pos = np.ascontiguousarray(positions, dtype=np.uint64)
    sn = None if sequence_numbers is None else np.ascontiguousarray(sequence_numbers, dtype=np.uint32)
    lengths = None if seed_lengths is None else np.ascontiguousarray(seed_lengths, dtype=np.uint32)
    n = max(o.size - 1, 0)
    names = [name for name, _ in CANDIDATE_SLOT_OUTPUTS + CANDIDATE_READ_OUTPUTS] + ["numOverflowed"]
    outputs = names if outputs is None else list(outputs)
    result = {}
    for name, dtype in CANDIDATE_SLOT_OUTPUTS + CANDIDATE_READ_OUTPUTS:
        if name in outputs:
            shape = (n, max_candidates) if (name, dtype) in CANDIDATE_SLOT_OUTPUTS else (n,)
            result[name] = np.zeros(shape, dtype)
            if fill is not None:
                result[name].view(np.uint8)[...] = fill
    overflowed = np.array([overflowed_before], np.uint64)

    def address(a):
        return a.ctypes.data if a is not None and a.size else None

    cin = candidate_inputs(address(o), ends.size if num_seeds is None else num_seeds, address(ends), address(lengths), fixed_length,
                           address(ho), pos.size if num_hits is None else num_hits, address(pos), address(sn))
    dummy = np.zeros(1, np.uint64)  # what an empty array points to: alive until the call has returned
    if lengths is not None and not lengths.size:  # (an empty array is still "lengths per seed")
        cin.seedLengths = dummy.ctypes.data
    cout = candidate_outputs(**{name: result[name].ctypes.data if result[name].size else dummy.ctypes.data for name in result})
    if "numOverflowed" in outputs:
        cout.numOverflowed = overflowed.ctypes.data
    rc = _lib.lib().awfmReadCandidates(C.byref(cin), n, max_hits_per_seed, band, min_votes, max_candidates, C.byref(cout), threads)
    _check("awfmReadCandidates", rc)
    if "numOverflowed" in outputs:
        result["numOverflowed"] = int(overflowed[0])
    return result


def read_candidates_scratch_bytes(n):
    """awfmGpuReadCandidatesScratchBytes: the bytes of device scratch GpuIndex.read_candidates needs for n reads"""
    return int(_lib.lib().awfmGpuReadCandidatesScratchBytes(n))


CHAINS_MAX_LOOKBACK = 64  # AWFM_CHAINS_MAX_LOOKBACK: the predecessors an anchor looks back at, at the most
CHAINS_NO_SLOT = 0xFFFFFFFF  # bestSlots of a read without an anchor
CHAIN_SLOT_OUTPUTS = (("chainScores", np.uint32), ("chainAnchors", np.uint32), ("chainReadBegins", np.uint32), ("chainReadEnds", np.uint32),
                      ("chainBeginDiagonals", np.int64), ("chainEndDiagonals", np.int64))
CHAIN_READ_OUTPUTS = (("bestSlots", np.uint32), ("keptHits", np.uint32))


def chain_outputs(**addresses):
    """struct AwFmChainOutputs from addresses by field name (chainScores, chainAnchors, chainReadBegins, chainReadEnds,
    chainBeginDiagonals, chainEndDiagonals, bestSlots, keptHits, numOverflowed); a field left out is NULL"""
    out = _lib.AwFmChainOutputs()
    for name, address in addresses.items():
        if name not in dict(_lib.AwFmChainOutputs._fields_):
            raise ValueError(f"no output called {name}")
        setattr(out, name, address or None)
    return out


def read_chains_host(read_seed_offsets, seed_ends, hit_offsets, positions, slot_sequences, slot_diagonals, slot_spans, sequence_numbers=None,
                     seed_lengths=None, fixed_length=0, max_hits_per_seed=0, band=0, lookback=CHAINS_MAX_LOOKBACK, gap_penalty=0, threads=4,
                     outputs=None, num_seeds=None, num_hits=None, fill=None, overflowed_before=0):
    """awfmReadChains (include/awfm_gpu.h, "read chains"): the inputs of read_candidates_host and the slot arrays it returned
    (sequences, diagonals, diagonalSpans, shaped (reads, max_candidates)) -> a dict of the outputs by field name: the six per-slot
    arrays shaped like the slots, bestSlots and keptHits per read, numOverflowed (an int: overflowed_before plus this call's).
    outputs: the names to compute (None: all); the others are passed as NULL and left out.  num_seeds / num_hits default to the
    arrays' sizes; fill: the value (per byte) the arrays hold before the call."""
    o = np.ascontiguousarray(read_seed_offsets, dtype=np.uint64)
    ends = np.ascontiguousarray(seed_ends, dtype=np.uint32)
    ho = np.ascontiguousarray(hit_offsets, dtype=np.uint64)
    pos = np.ascontiguousarray(positions, dtype=np.uint64)
    sn = None if sequence_numbers is None else np.ascontiguousarray(sequence_numbers, dtype=np.uint32)
    lengths = None if seed_lengths is None else np.ascontiguousarray(seed_lengths, dtype=np.uint32)
    n = max(o.size - 1, 0)
    slot_seq = np.ascontiguousarray(slot_sequences, dtype=np.uint32)
    slot_diag = np.ascontiguousarray(slot_diagonals, dtype=np.int64)
    slot_span = np.ascontiguousarray(slot_spans, dtype=np.uint32)
    if slot_seq.ndim != 2 or slot_seq.shape[0] != n or slot_diag.shape != slot_seq.shape or slot_span.shape != slot_seq.shape:
        raise ValueError("the slot arrays are shaped (reads, max_candidates)")
    max_candidates = slot_seq.shape[1]
    names = [name for name, _ in CHAIN_SLOT_OUTPUTS + CHAIN_READ_OUTPUTS] + ["numOverflowed"]
    outputs = names if outputs is None else list(outputs)
    result = {}
    for name, dtype in CHAIN_SLOT_OUTPUTS + CHAIN_READ_OUTPUTS:
        if name in outputs:
            shape = (n, max_candidates) if (name, dtype) in CHAIN_SLOT_OUTPUTS else (n,)
            result[name] = np.zeros(shape, dtype)
            if fill is not None:
                result[name].view(np.uint8)[...] = fill
    overflowed = np.array([overflowed_before], np.uint64)
    dummy = np.zeros(1, np.uint64)  # what an empty array points to: alive until the call has returned

    def address(a):
        return a.ctypes.data if a is not None and a.size else None

    cin = candidate_inputs(address(o), ends.size if num_seeds is None else num_seeds, address(ends), address(lengths), fixed_length,
                           address(ho), pos.size if num_hits is None else num_hits, address(pos), address(sn))
    if lengths is not None and not lengths.size:  # (an empty array is still "lengths per seed")
        cin.seedLengths = dummy.ctypes.data
    cout = chain_outputs(**{name: result[name].ctypes.data if result[name].size else dummy.ctypes.data for name in result})
    if "numOverflowed" in outputs:
        cout.numOverflowed = overflowed.ctypes.data
    rc = _lib.lib().awfmReadChains(C.byref(cin), n, max_hits_per_seed, band, max_candidates, address(slot_seq) or dummy.ctypes.data,
                                   address(slot_diag) or dummy.ctypes.data, address(slot_span) or dummy.ctypes.data, lookback, gap_penalty,
                                   C.byref(cout), threads)
    _check("awfmReadChains", rc)
    if "numOverflowed" in outputs:
        result["numOverflowed"] = int(overflowed[0])
    return result


def read_chains_scratch_bytes(n):
    """awfmGpuReadChainsScratchBytes: the bytes of device scratch GpuIndex.read_chains needs for n reads"""
    return int(_lib.lib().awfmGpuReadChainsScratchBytes(n))


VERIFY_MAX_BAND = 64  # AWFM_VERIFY_MAX_BAND: maxDrift + 2 bandPad + 1 diagonals at the most
VERIFY_MAX_LENGTH = 1 << 20  # AWFM_VERIFY_MAX_LENGTH: read characters of a chain that is verified
VERIFY_NONE, VERIFY_MALFORMED, VERIFY_TOO_WIDE, VERIFY_TOO_LONG = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
VERIFY_SLOT_INPUTS = (("sequences", np.uint32), ("chainAnchors", np.uint32), ("chainReadBegins", np.uint32), ("chainReadEnds", np.uint32),
                      ("chainBeginDiagonals", np.int64), ("chainEndDiagonals", np.int64))


def verify_inputs(read_chars, num_read_chars, read_offsets, **slot_addresses):
    """struct AwFmVerifyInputs from addresses: the read buffer, its size, the read offsets, and the six per-slot arrays by field
    name (sequences, chainAnchors, chainReadBegins, chainReadEnds, chainBeginDiagonals, chainEndDiagonals)"""
    vin = _lib.AwFmVerifyInputs(read_chars or None, num_read_chars, read_offsets or None)
    for name, address in slot_addresses.items():
        if name not in dict(VERIFY_SLOT_INPUTS):
            raise ValueError(f"no slot array called {name}")
        setattr(vin, name, address or None)
    return vin


def verify_outputs(**addresses):
    """struct AwFmVerifyOutputs from addresses by field name (editDistances, bestSlots, numUnverified); a field left out is NULL"""
    out = _lib.AwFmVerifyOutputs()
    for name, address in addresses.items():
        if name not in dict(_lib.AwFmVerifyOutputs._fields_):
            raise ValueError(f"no output called {name}")
        setattr(out, name, address or None)
    return out


def text_windows_host(text, positions, before, after, threads=4):
    """awfmTextWindows: text (bytes or uint8 array), positions -> uint8 array shaped (positions, before + after): window i is
    text[p - before, p + after) with every byte outside the text written as 0"""
    t = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    pos = np.ascontiguousarray(positions, dtype=np.uint64)
    out = np.full((pos.size, max(before + after, 0)), 0xAA, np.uint8)
    dummy = np.zeros(1, np.uint64)
    rc = _lib.lib().awfmTextWindows(t.ctypes.data if t.size else None, t.size, pos.ctypes.data if pos.size else dummy.ctypes.data, pos.size,
                                    before, after, out.ctypes.data if out.size else dummy.ctypes.data, threads)
    _check("awfmTextWindows", rc)
    return out


def verify_chains_host(read_chars, read_offsets, slots, text, sequence_ends=None, alphabet=AwFmAlphabetDna, band_pad=8, max_drift=15,
                       threads=4, outputs=None, num_read_chars=None, fill=None, unverified_before=0):
    """awfmVerifyChains (include/awfm_gpu.h, "chain verification"): the read buffer and offsets, `slots` a dict of the six per-slot
    arrays by field name shaped (reads, max_candidates), the text and the records' ends (None: one sequence) -> a dict of
    editDistances shaped like the slots, bestSlots per read and numUnverified (an int: unverified_before plus this call's).
    outputs: the names to compute (None: all); the others are passed as NULL and left out.  fill: the value (per byte) the
    arrays hold before the call."""
    chars = np.frombuffer(read_chars, np.uint8) if isinstance(read_chars, (bytes, bytearray)) else np.ascontiguousarray(read_chars, dtype=np.uint8)
    t = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    o = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    ends = None if sequence_ends is None else np.ascontiguousarray(sequence_ends, dtype=np.uint64)
    n = max(o.size - 1, 0)
    arrays = {name: np.ascontiguousarray(slots[name], dtype=dtype) for name, dtype in VERIFY_SLOT_INPUTS}
    shape = arrays["sequences"].shape
    if len(shape) != 2 or shape[0] != n or any(a.shape != shape for a in arrays.values()):
        raise ValueError("the slot arrays are shaped (reads, max_candidates)")
    names = ["editDistances", "bestSlots", "numUnverified"]
    outputs = names if outputs is None else list(outputs)
    result = {}
    if "editDistances" in outputs:
        result["editDistances"] = np.zeros(shape, np.uint32)
    if "bestSlots" in outputs:
        result["bestSlots"] = np.zeros(n, np.uint32)
    for a in result.values():
        if fill is not None:
            a.view(np.uint8)[...] = fill
    unverified = np.array([unverified_before], np.uint64)
    dummy = np.zeros(1, np.uint64)  # what an empty array points to: alive until the call has returned

    def address(a):
        return a.ctypes.data if a is not None and a.size else dummy.ctypes.data

    vin = verify_inputs(address(chars), chars.size if num_read_chars is None else num_read_chars, address(o),
                        **{name: address(a) for name, a in arrays.items()})
    vout = verify_outputs(**{name: address(a) for name, a in result.items()})
    if "numUnverified" in outputs:
        vout.numUnverified = unverified.ctypes.data
    rc = _lib.lib().awfmVerifyChains(C.byref(vin), n, shape[1], band_pad, max_drift, address(t), t.size,
                                     None if ends is None or not ends.size else ends.ctypes.data, 0 if ends is None else ends.size, alphabet,
                                     C.byref(vout), threads)
    _check("awfmVerifyChains", rc)
    if "numUnverified" in outputs:
        result["numUnverified"] = int(unverified[0])
    return result


ALIGN_MAX_LENGTH = 1 << 16  # AWFM_ALIGN_MAX_LENGTH: read characters per aligned read
ALIGN_MAX_OPS = 4096  # AWFM_ALIGN_MAX_OPS: upper limit of max_ops
ALIGN_OVERHANG = 0xFFFFFFFB  # AWFM_ALIGN_OVERHANG, beside VERIFY_NONE .. VERIFY_TOO_LONG
ALIGN_OP_LETTERS = {1: "I", 2: "D", 4: "S", 7: "=", 8: "X"}  # BAM numbering of the operations a run carries in its low four bits
ALIGN_READ_OUTPUTS = (("editDistances", np.uint32), ("textBegins", np.uint64), ("textEnds", np.uint64), ("numOps", np.uint32))


def align_outputs(**addresses):
    """struct AwFmAlignOutputs from addresses by field name (editDistances, textBegins, textEnds, numOps, ops, numUnaligned,
    numTruncated); a field left out is NULL"""
    out = _lib.AwFmAlignOutputs()
    for name, address in addresses.items():
        if name not in dict(_lib.AwFmAlignOutputs._fields_):
            raise ValueError(f"no output called {name}")
        setattr(out, name, address or None)
    return out


def cigar_of(ops):
    """the text form of a row of runs (run << 4 | op)"""
    return "".join(f"{int(v) >> 4}{ALIGN_OP_LETTERS[int(v) & 15]}" for v in ops)


def align_chains_host(read_chars, read_offsets, slots, chosen, text, sequence_ends=None, alphabet=AwFmAlphabetDna, band_pad=8, max_drift=15,
                      max_ops=32, threads=4, outputs=None, num_read_chars=None, fill=None, unaligned_before=0, truncated_before=0):
    """awfmAlignChains (include/awfm_gpu.h, "chain alignment"): the inputs of verify_chains_host and `chosen`, the slot of every
    read to align -> a dict of editDistances, textBegins, textEnds, numOps per read, ops shaped (reads, max_ops), numUnaligned and
    numTruncated (ints: the values before plus this call's).  outputs: the names to compute (None: all); the others are passed as
    NULL and left out.  fill: the value (per byte) the arrays hold before the call."""
    chars = np.frombuffer(read_chars, np.uint8) if isinstance(read_chars, (bytes, bytearray)) else np.ascontiguousarray(read_chars, dtype=np.uint8)
    t = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    o = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    ends = None if sequence_ends is None else np.ascontiguousarray(sequence_ends, dtype=np.uint64)
    n = max(o.size - 1, 0)
    arrays = {name: np.ascontiguousarray(slots[name], dtype=dtype) for name, dtype in VERIFY_SLOT_INPUTS}
    shape = arrays["sequences"].shape
    which = np.ascontiguousarray(chosen, dtype=np.uint32)
    if len(shape) != 2 or shape[0] != n or any(a.shape != shape for a in arrays.values()) or which.shape != (n,):
        raise ValueError("the slot arrays are shaped (reads, max_candidates), the chosen slots (reads,)")
    names = [name for name, _ in ALIGN_READ_OUTPUTS] + ["ops", "numUnaligned", "numTruncated"]
    outputs = names if outputs is None else list(outputs)
    result = {name: np.zeros(n, dtype) for name, dtype in ALIGN_READ_OUTPUTS if name in outputs}
    if "ops" in outputs:
        result["ops"] = np.zeros((n, max(int(max_ops), 0)), np.uint32)
    for a in result.values():
        if fill is not None:
            a.view(np.uint8)[...] = fill
    counters = {"numUnaligned": np.array([unaligned_before], np.uint64), "numTruncated": np.array([truncated_before], np.uint64)}
    dummy = np.zeros(1, np.uint64)  # what an empty array points to: alive until the call has returned

    def address(a):
        return a.ctypes.data if a is not None and a.size else dummy.ctypes.data

    vin = verify_inputs(address(chars), chars.size if num_read_chars is None else num_read_chars, address(o),
                        **{name: address(a) for name, a in arrays.items()})
    aout = align_outputs(**{name: address(a) for name, a in result.items()})
    for name, counter in counters.items():
        if name in outputs:
            setattr(aout, name, counter.ctypes.data)
    rc = _lib.lib().awfmAlignChains(C.byref(vin), address(which), n, shape[1], band_pad, max_drift, max_ops, address(t), t.size,
                                    None if ends is None or not ends.size else ends.ctypes.data, 0 if ends is None else ends.size, alphabet,
                                    C.byref(aout), threads)
    _check("awfmAlignChains", rc)
    for name, counter in counters.items():
        if name in outputs:
            result[name] = int(counter[0])
    return result


AFFINE_READ_OUTPUTS = (("scores", np.uint32), ("editDistances", np.uint32), ("readBegins", np.uint32), ("readEnds", np.uint32),
                       ("textBegins", np.uint64), ("textEnds", np.uint64), ("numOps", np.uint32))
AFFINE_SCORING = (1, 4, 6, 1)  # match, mismatch, gapOpen, gapExtend: the scoring of the examples and the measurements


def align_scoring(match=1, mismatch=4, gap_open=6, gap_extend=1):
    """struct AwFmAlignScoring: a gap of g characters costs gap_open + g * gap_extend"""
    return _lib.AwFmAlignScoring(match, mismatch, gap_open, gap_extend)


MATRIX_CLASSES = 21  # AWFM_MATRIX_CLASSES


END_BONUS = 5         # the end bonus the *_end_bonus calls take by default: BWA-MEM's clip penalty
END_BONUS_MAX = 255   # AWFM_END_BONUS_MAX


def matrix_scoring(substitution, gap_open=6, gap_extend=1):
    """struct AwFmMatrixScoring (include/awfm_gpu.h, "substitution matrices") from 21 x 21 int8 values, [class of the read's character,
    class of the text's], and the gap costs"""
    values = np.ascontiguousarray(substitution)
    if values.shape != (MATRIX_CLASSES, MATRIX_CLASSES) or (values < -128).any() or (values > 127).any():
        raise ValueError("a substitution matrix is 21 x 21 values of -128 .. 127")
    out = _lib.AwFmMatrixScoring()
    out.substitution[:] = [int(v) for v in values.reshape(-1)]
    out.gapOpen, out.gapExtend = gap_open, gap_extend
    return out


def matrix_values(matrix):
    """the 21 x 21 values of a struct AwFmMatrixScoring as an int8 array"""
    return np.array(matrix.substitution[:], np.int8).reshape(MATRIX_CLASSES, MATRIX_CLASSES)


def matrix_scoring_uniform(alphabet=AwFmAlphabetDna, scoring=AFFINE_SCORING):
    """awfmMatrixScoringUniform: the matrix under which the matrix calls equal the affine ones under `scoring`"""
    costs = scoring if isinstance(scoring, _lib.AwFmAlignScoring) else align_scoring(*scoring)
    out = _lib.AwFmMatrixScoring()
    _check("awfmMatrixScoringUniform", _lib.lib().awfmMatrixScoringUniform(alphabet, C.byref(costs), C.byref(out)))
    return out


def matrix_scoring_from_text(text, alphabet=AwFmAlphabetAmino, gap_open=11, gap_extend=1, num_bytes=None):
    """awfmMatrixScoringFromText: the usual matrix text format (bytes or str; num_bytes: only that many of them) -> a struct
    AwFmMatrixScoring"""
    data = text.encode() if isinstance(text, str) else bytes(text)
    size = len(data) if num_bytes is None else num_bytes
    block = np.frombuffer(data[:size], np.uint8).copy()  # exactly the bytes the call may read
    out = _lib.AwFmMatrixScoring()
    _check("awfmMatrixScoringFromText", _lib.lib().awfmMatrixScoringFromText(alphabet, block.ctypes.data if size else None, size, gap_open,
                                                                              gap_extend, C.byref(out)))
    return out


def affine_outputs(**addresses):
    """struct AwFmAffineOutputs from addresses by field name (scores, editDistances, readBegins, readEnds, textBegins, textEnds,
    numOps, ops, numUnaligned, numTruncated); a field left out is NULL"""
    out = _lib.AwFmAffineOutputs()
    for name, address in addresses.items():
        if name not in dict(_lib.AwFmAffineOutputs._fields_):
            raise ValueError(f"no output called {name}")
        setattr(out, name, address or None)
    return out


def align_chains_affine_host(read_chars, read_offsets, slots, chosen, text, sequence_ends=None, alphabet=AwFmAlphabetDna, band_pad=8,
                             max_drift=15, scoring=AFFINE_SCORING, max_ops=32, threads=4, outputs=None, num_read_chars=None, fill=None,
                             unaligned_before=0, truncated_before=0):
    """awfmAlignChainsAffine (include/awfm_gpu.h, "affine alignment"): the inputs of align_chains_host and `scoring` = (match,
    mismatch, gap_open, gap_extend) -> a dict of scores, editDistances, readBegins, readEnds, textBegins, textEnds, numOps per read,
    ops shaped (reads, max_ops), numUnaligned and numTruncated (ints: the values before plus this call's).  outputs: the names to
    compute (None: all); the others are passed as NULL and left out.  fill: the value (per byte) the arrays hold before the call."""
    costs = scoring if isinstance(scoring, _lib.AwFmAlignScoring) else align_scoring(*scoring)
    return _align_chains_scored_host("awfmAlignChainsAffine", costs, read_chars, read_offsets, slots, chosen, text, sequence_ends, alphabet,
                                     band_pad, max_drift, max_ops, threads, outputs, num_read_chars, fill, unaligned_before, truncated_before)


def align_chains_matrix_host(read_chars, read_offsets, slots, chosen, text, matrix, sequence_ends=None, alphabet=AwFmAlphabetDna, band_pad=8,
                             max_drift=15, max_ops=32, threads=4, outputs=None, num_read_chars=None, fill=None, unaligned_before=0,
                             truncated_before=0):
    """awfmAlignChainsMatrix (include/awfm_gpu.h, "substitution matrices"): align_chains_affine_host with a matrix_scoring(...) in
    place of the scoring (None: the call's NULL)"""
    return _align_chains_scored_host("awfmAlignChainsMatrix", matrix, read_chars, read_offsets, slots, chosen, text, sequence_ends, alphabet,
                                     band_pad, max_drift, max_ops, threads, outputs, num_read_chars, fill, unaligned_before, truncated_before)


def align_chains_end_bonus_host(read_chars, read_offsets, slots, chosen, text, matrix, end_bonus=END_BONUS, sequence_ends=None,
                                alphabet=AwFmAlphabetDna, band_pad=8, max_drift=15, max_ops=32, threads=4, outputs=None, num_read_chars=None,
                                fill=None, unaligned_before=0, truncated_before=0):
    """awfmAlignChainsEndBonus (include/awfm_gpu.h, "end bonus"): align_chains_matrix_host with end_bonus, 0 to 255, earned by an
    alignment at each read end it reaches; the scores include it"""
    return _align_chains_scored_host("awfmAlignChainsEndBonus", matrix, read_chars, read_offsets, slots, chosen, text, sequence_ends, alphabet,
                                     band_pad, max_drift, max_ops, threads, outputs, num_read_chars, fill, unaligned_before, truncated_before,
                                     behind=(end_bonus,))


def _align_chains_scored_host(symbol, costs, read_chars, read_offsets, slots, chosen, text, sequence_ends, alphabet, band_pad, max_drift, max_ops,
                              threads, outputs, num_read_chars, fill, unaligned_before, truncated_before, behind=()):
    """the calls above: `symbol` with `costs`, the struct it takes, and what the call takes behind it"""
    chars = np.frombuffer(read_chars, np.uint8) if isinstance(read_chars, (bytes, bytearray)) else np.ascontiguousarray(read_chars, dtype=np.uint8)
    t = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    o = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    ends = None if sequence_ends is None else np.ascontiguousarray(sequence_ends, dtype=np.uint64)
    n = max(o.size - 1, 0)
    arrays = {name: np.ascontiguousarray(slots[name], dtype=dtype) for name, dtype in VERIFY_SLOT_INPUTS}
    shape = arrays["sequences"].shape
    which = np.ascontiguousarray(chosen, dtype=np.uint32)
    if len(shape) != 2 or shape[0] != n or any(a.shape != shape for a in arrays.values()) or which.shape != (n,):
        raise ValueError("the slot arrays are shaped (reads, max_candidates), the chosen slots (reads,)")
    names = [name for name, _ in AFFINE_READ_OUTPUTS] + ["ops", "numUnaligned", "numTruncated"]
    outputs = names if outputs is None else list(outputs)
    result = {name: np.zeros(n, dtype) for name, dtype in AFFINE_READ_OUTPUTS if name in outputs}
    if "ops" in outputs:
        result["ops"] = np.zeros((n, max(int(max_ops), 0)), np.uint32)
    for a in result.values():
        if fill is not None:
            a.view(np.uint8)[...] = fill
    counters = {"numUnaligned": np.array([unaligned_before], np.uint64), "numTruncated": np.array([truncated_before], np.uint64)}
    dummy = np.zeros(1, np.uint64)  # what an empty array points to: alive until the call has returned

    def address(a):
        return a.ctypes.data if a is not None and a.size else dummy.ctypes.data

    vin = verify_inputs(address(chars), chars.size if num_read_chars is None else num_read_chars, address(o),
                        **{name: address(a) for name, a in arrays.items()})
    aout = affine_outputs(**{name: address(a) for name, a in result.items()})
    for name, counter in counters.items():
        if name in outputs:
            setattr(aout, name, counter.ctypes.data)
    rc = getattr(_lib.lib(), symbol)(C.byref(vin), address(which), n, shape[1], band_pad, max_drift, None if costs is None else C.byref(costs),
                                     *behind, max_ops, address(t), t.size, None if ends is None or not ends.size else ends.ctypes.data,
                                     0 if ends is None else ends.size, alphabet, C.byref(aout), threads)
    _check(symbol, rc)
    for name, counter in counters.items():
        if name in outputs:
            result[name] = int(counter[0])
    return result


STRINGS_CIGAR_M = 1  # AWFM_STRINGS_CIGAR_M: the classic CIGAR, '=' and 'X' merged into M
STRING_INPUTS = (("sequences", np.uint32), ("slots", np.uint32), ("textBegins", np.uint64), ("numOps", np.uint32), ("ops", np.uint32))


def string_inputs(sequences, slots, text_begins, num_ops, ops):
    """struct AwFmStringInputs (include/awfm_gpu.h, "alignment strings") from five addresses, host or device: the slot table's
    sequences, the slots the alignment call was given, and its textBegins, numOps and ops"""
    return _lib.AwFmStringInputs(sequences or None, slots or None, text_begins or None, num_ops or None, ops or None)


def string_outputs(**addresses):
    """struct AwFmStringOutputs from addresses by field name (cigarOffsets, cigarChars, mdOffsets, mdChars, numSkipped,
    numOverflow) and the two capacities (cigarCapacity, mdCapacity); a field left out is NULL or 0"""
    out = _lib.AwFmStringOutputs()
    for name, value in addresses.items():
        if name not in dict(_lib.AwFmStringOutputs._fields_):
            raise ValueError(f"no output called {name}")
        setattr(out, name, int(value) if name.endswith("Capacity") else (value or None))
    return out


def strings_of(offsets, chars):
    """the strings of a packed arena as a list of bytes: read r's is chars[offsets[r] : offsets[r + 1]]"""
    data = np.ascontiguousarray(chars, dtype=np.uint8).tobytes()
    return [data[int(offsets[r]):int(offsets[r + 1])] for r in range(len(offsets) - 1)]


def alignment_strings_host(sequences, slots, text_begins, num_ops, ops, text, sequence_ends=None, alphabet=AwFmAlphabetDna, classic=False,
                           cigar_capacity=None, md_capacity=None, outputs=None, threads=4, fill=None, skipped_before=0, overflow_before=0,
                           flags=None, max_candidates=None, max_ops=None):
    """awfmAlignmentStrings (include/awfm_gpu.h, "alignment strings"), the host twin: sequences shaped (reads, max_candidates), slots,
    text_begins and num_ops per read, ops shaped (reads, max_ops) -> a dict of cigarOffsets, mdOffsets (uint64, reads + 1),
    cigarChars, mdChars (uint8 arenas of the capacity given; None: exactly what the strings need, found by a first call for the
    offsets), numSkipped and numOverflow (ints: the values before plus this call's).  outputs: the names to compute (None: all);
    the others are passed as NULL and left out.  fill: the value (per byte) the arrays hold before the call."""
    seq = np.ascontiguousarray(sequences, dtype=np.uint32)
    arrays = {"sequences": seq, "slots": np.ascontiguousarray(slots, dtype=np.uint32), "textBegins": np.ascontiguousarray(text_begins, dtype=np.uint64),
              "numOps": np.ascontiguousarray(num_ops, dtype=np.uint32), "ops": np.ascontiguousarray(ops, dtype=np.uint32)}
    n = arrays["slots"].size
    if seq.ndim != 2 or seq.shape[0] != n or arrays["ops"].ndim != 2 or arrays["ops"].shape[0] != n or arrays["textBegins"].shape != (n,) \
            or arrays["numOps"].shape != (n,):
        raise ValueError("sequences is shaped (reads, max_candidates), ops (reads, max_ops), the others (reads,)")
    t = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    ends = None if sequence_ends is None else np.ascontiguousarray(sequence_ends, dtype=np.uint64)
    C_ = seq.shape[1] if max_candidates is None else max_candidates
    M_ = arrays["ops"].shape[1] if max_ops is None else max_ops
    flags = (STRINGS_CIGAR_M if classic else 0) if flags is None else flags
    names = ["cigarOffsets", "cigarChars", "mdOffsets", "mdChars", "numSkipped", "numOverflow"]
    outputs = names if outputs is None else list(outputs)
    dummy = np.zeros(1, np.uint64)  # what an empty array points to: alive until the call has returned

    def address(a):
        return a.ctypes.data if a is not None and a.size else dummy.ctypes.data

    sin = string_inputs(*(address(arrays[name]) for name, _ in STRING_INPUTS))

    def call(sout):
        rc = _lib.lib().awfmAlignmentStrings(C.byref(sin), n, C_, M_, flags, address(t), t.size,
                                             None if ends is None or not ends.size else ends.ctypes.data, 0 if ends is None else ends.size,
                                             alphabet, C.byref(sout), threads)
        _check("awfmAlignmentStrings", rc)

    if (cigar_capacity is None and "cigarChars" in outputs) or (md_capacity is None and "mdChars" in outputs):
        sizing = {"cigarOffsets": np.zeros(n + 1, np.uint64), "mdOffsets": np.zeros(n + 1, np.uint64)}
        call(string_outputs(**{name: a.ctypes.data for name, a in sizing.items()}))
        cigar_capacity = int(sizing["cigarOffsets"][n]) if cigar_capacity is None else cigar_capacity
        md_capacity = int(sizing["mdOffsets"][n]) if md_capacity is None else md_capacity
    result = {}
    for name, size, dtype in (("cigarOffsets", n + 1, np.uint64), ("cigarChars", cigar_capacity or 0, np.uint8), ("mdOffsets", n + 1, np.uint64),
                              ("mdChars", md_capacity or 0, np.uint8)):
        if name in outputs:
            result[name] = np.zeros(size, dtype)
            if fill is not None:
                result[name].view(np.uint8)[...] = fill
    counters = {"numSkipped": np.array([skipped_before], np.uint64), "numOverflow": np.array([overflow_before], np.uint64)}
    sout = string_outputs(cigarCapacity=cigar_capacity or 0, mdCapacity=md_capacity or 0, **{name: address(a) for name, a in result.items()})
    for name, counter in counters.items():
        if name in outputs:
            setattr(sout, name, counter.ctypes.data)
    call(sout)
    for name, counter in counters.items():
        if name in outputs:
            result[name] = int(counter[0])
    return result


SAM_PAIRED = 1  # AWFM_SAM_PAIRED: reads 2p and 2p + 1 are mates
# field name, element type, required; in the order of struct AwFmSamInputs (numReadChars and numRecordNames are numbers)
SAM_INPUTS = (("readChars", np.uint8, True), ("readOffsets", np.uint64, True), ("qualities", np.uint8, False), ("nameOffsets", np.uint64, False),
              ("nameChars", np.uint8, False), ("recordNameOffsets", np.uint64, True), ("recordNameChars", np.uint8, True),
              ("sequences", np.uint32, True), ("slots", np.uint32, True), ("scores", np.uint32, True), ("editDistances", np.uint32, True),
              ("textBegins", np.uint64, True), ("textEnds", np.uint64, True), ("cigarOffsets", np.uint64, True), ("cigarChars", np.uint8, True),
              ("mdOffsets", np.uint64, False), ("mdChars", np.uint8, False), ("mappingQualities", np.uint8, False),
              ("secondScores", np.uint32, False), ("baseFlags", np.uint16, False), ("properPairs", np.uint8, False))


def sam_inputs(num_read_chars=0, num_record_names=0, **addresses):
    """struct AwFmSamInputs (include/awfm_gpu.h, "SAM records") from addresses by field name, host or device, and the two numbers;
    a field left out is NULL"""
    sin = _lib.AwFmSamInputs()
    sin.numReadChars, sin.numRecordNames = int(num_read_chars), int(num_record_names)
    known = {name for name, _, _ in SAM_INPUTS}
    for name, value in addresses.items():
        if name not in known:
            raise ValueError(f"no input called {name}")
        setattr(sin, name, value or None)
    return sin


def sam_outputs(**addresses):
    """struct AwFmSamOutputs from addresses by field name (lineOffsets, lineChars, numUnaligned, numOverflow) and lineCapacity; a
    field left out is NULL or 0"""
    out = _lib.AwFmSamOutputs()
    for name, value in addresses.items():
        if name not in dict(_lib.AwFmSamOutputs._fields_):
            raise ValueError(f"no output called {name}")
        setattr(out, name, int(value) if name == "lineCapacity" else (value or None))
    return out


def sam_records_host(arrays, max_candidates=None, paired=False, line_capacity=None, outputs=None, threads=4, fill=None, unaligned_before=0,
                     overflow_before=0, flags=None, num_reads=None, num_record_names=None):
    """awfmSamRecords (include/awfm_gpu.h, "SAM records"), the host twin: arrays is a dict by the field names of struct
    AwFmSamInputs (SAM_INPUTS; sequences shaped (reads, max_candidates); an optional one left out or None is NULL) -> a dict of
    lineOffsets (uint64, reads + 1), lineChars (a uint8 arena of the capacity given; None: exactly what the lines need, found by
    a first call for the offsets), numUnaligned and numOverflow (ints: the values before plus this call's).  outputs: the names to
    compute (None: all); the others are passed as NULL and left out.  fill: the value (per byte) the arrays hold before the
    call."""
    held = {}
    for name, dtype, _ in SAM_INPUTS:
        if arrays.get(name) is not None:
            held[name] = np.ascontiguousarray(arrays[name], dtype=dtype)
    n = (held["readOffsets"].size - 1 if "readOffsets" in held else 0) if num_reads is None else num_reads
    C_ = (held["sequences"].shape[1] if "sequences" in held and held["sequences"].ndim == 2 else 1) if max_candidates is None else max_candidates
    records = (held["recordNameOffsets"].size - 1 if "recordNameOffsets" in held else 0) if num_record_names is None else num_record_names
    flags = (SAM_PAIRED if paired else 0) if flags is None else flags
    dummy = np.zeros(1, np.uint64)  # what an empty array points to: alive until the call has returned

    def address(a):
        return a.ctypes.data if a.size else dummy.ctypes.data

    sin = sam_inputs(held["readChars"].size if "readChars" in held else 0, records, **{name: address(a) for name, a in held.items()})
    names = ["lineOffsets", "lineChars", "numUnaligned", "numOverflow"]
    outputs = names if outputs is None else list(outputs)

    def call(sout):
        _check("awfmSamRecords", _lib.lib().awfmSamRecords(C.byref(sin), n, C_, flags, C.byref(sout), threads))

    if line_capacity is None and "lineChars" in outputs:
        sizing = np.zeros(n + 1, np.uint64)
        call(sam_outputs(lineOffsets=sizing.ctypes.data))
        line_capacity = int(sizing[n])
    result = {}
    for name, size, dtype in (("lineOffsets", n + 1, np.uint64), ("lineChars", line_capacity or 0, np.uint8)):
        if name in outputs:
            result[name] = np.zeros(size, dtype)
            if fill is not None:
                result[name].view(np.uint8)[...] = fill
    counters = {"numUnaligned": np.array([unaligned_before], np.uint64), "numOverflow": np.array([overflow_before], np.uint64)}
    sout = sam_outputs(lineCapacity=line_capacity or 0, **{name: address(a) for name, a in result.items()})
    for name, counter in counters.items():
        if name in outputs:
            setattr(sout, name, counter.ctypes.data)
    call(sout)
    for name, counter in counters.items():
        if name in outputs:
            result[name] = int(counter[0])
    return result


def record_names(index):
    """awfmRecordNames: the first whitespace-delimited token of every record's header -> (offsets uint64 [records + 1], chars
    uint8), what sam_records takes as recordNameOffsets and recordNameChars"""
    records = int(_lib.lib().awFmGetNumSequences(index.ptr))
    offsets = np.zeros(records + 1, np.uint64)
    _check("awfmRecordNames", _lib.lib().awfmRecordNames(index.ptr, offsets.ctypes.data, None, 0))
    chars = np.zeros(max(int(offsets[records]), 1), np.uint8)
    _check("awfmRecordNames", _lib.lib().awfmRecordNames(index.ptr, offsets.ctypes.data, chars.ctypes.data, int(offsets[records])))
    return offsets, chars[:int(offsets[records])]


def sam_header(index):
    """awfmSamHeader: the @HD line and one @SQ line per record of the index, as bytes (empty without records)"""
    size = int(_lib.lib().awfmSamHeader(index.ptr, None, 0))
    out = np.zeros(max(size, 1), np.uint8)
    _lib.lib().awfmSamHeader(index.ptr, out.ctypes.data, size)
    return out[:size].tobytes()


SCORE_MAX_MAPQ = 254  # AWFM_SCORE_MAX_MAPQ: upper limit of mapq_cap (255 is SAM's "unavailable")
SCORE_SLOT_OUTPUTS = (("slotScores", np.uint32), ("slotReadEnds", np.uint32), ("slotTextEnds", np.uint64))
SCORE_READ_OUTPUTS = (("bestSlots", np.uint32), ("bestScores", np.uint32), ("secondSlots", np.uint32), ("secondScores", np.uint32),
                      ("mappingQualities", np.uint8))


def slot_score_outputs(**addresses):
    """struct AwFmSlotScoreOutputs from addresses by field name (slotScores, slotReadEnds, slotTextEnds, bestSlots, bestScores,
    secondSlots, secondScores, mappingQualities, numUnscored, numMapped); a field left out is NULL"""
    out = _lib.AwFmSlotScoreOutputs()
    for name, address in addresses.items():
        if name not in dict(_lib.AwFmSlotScoreOutputs._fields_):
            raise ValueError(f"no output called {name}")
        setattr(out, name, address or None)
    return out


def score_chains_affine_host(read_chars, read_offsets, slots, text, sequence_ends=None, alphabet=AwFmAlphabetDna, band_pad=8, max_drift=15,
                             scoring=AFFINE_SCORING, min_score=0, mapq_cap=60, threads=4, outputs=None, num_read_chars=None, fill=None,
                             unscored_before=0, mapped_before=0):
    """awfmScoreChainsAffine (include/awfm_gpu.h, "slot scores and mapping quality"): the inputs of verify_chains_host and `scoring`
    = (match, mismatch, gap_open, gap_extend) -> a dict of slotScores, slotReadEnds, slotTextEnds shaped like the slots, bestSlots,
    bestScores, secondSlots, secondScores, mappingQualities per read, numUnscored and numMapped (ints: the values before plus this
    call's).  outputs: the names to compute (None: all); the others are passed as NULL and left out.  fill: the value (per byte)
    the arrays hold before the call."""
    costs = scoring if isinstance(scoring, _lib.AwFmAlignScoring) else align_scoring(*scoring)
    return _score_chains_scored_host("awfmScoreChainsAffine", costs, read_chars, read_offsets, slots, text, sequence_ends, alphabet, band_pad,
                                     max_drift, min_score, mapq_cap, threads, outputs, num_read_chars, fill, unscored_before, mapped_before)


def score_chains_matrix_host(read_chars, read_offsets, slots, text, matrix, sequence_ends=None, alphabet=AwFmAlphabetDna, band_pad=8, max_drift=15,
                             min_score=0, mapq_cap=60, threads=4, outputs=None, num_read_chars=None, fill=None, unscored_before=0,
                             mapped_before=0):
    """awfmScoreChainsMatrix (include/awfm_gpu.h, "substitution matrices"): score_chains_affine_host with a matrix_scoring(...) in
    place of the scoring (None: the call's NULL)"""
    return _score_chains_scored_host("awfmScoreChainsMatrix", matrix, read_chars, read_offsets, slots, text, sequence_ends, alphabet, band_pad,
                                     max_drift, min_score, mapq_cap, threads, outputs, num_read_chars, fill, unscored_before, mapped_before)


def score_chains_end_bonus_host(read_chars, read_offsets, slots, text, matrix, end_bonus=END_BONUS, sequence_ends=None, alphabet=AwFmAlphabetDna,
                                band_pad=8, max_drift=15, min_score=0, mapq_cap=60, threads=4, outputs=None, num_read_chars=None, fill=None,
                                unscored_before=0, mapped_before=0):
    """awfmScoreChainsEndBonus (include/awfm_gpu.h, "end bonus"): score_chains_matrix_host with end_bonus, 0 to 255; the slot scores,
    min_score and the mapping quality work on scores that include it"""
    return _score_chains_scored_host("awfmScoreChainsEndBonus", matrix, read_chars, read_offsets, slots, text, sequence_ends, alphabet, band_pad,
                                     max_drift, min_score, mapq_cap, threads, outputs, num_read_chars, fill, unscored_before, mapped_before,
                                     behind=(end_bonus,))


def _score_chains_scored_host(symbol, costs, read_chars, read_offsets, slots, text, sequence_ends, alphabet, band_pad, max_drift, min_score,
                              mapq_cap, threads, outputs, num_read_chars, fill, unscored_before, mapped_before, behind=()):
    """the calls above: `symbol` with `costs`, the struct it takes, and what the call takes behind it"""
    chars = np.frombuffer(read_chars, np.uint8) if isinstance(read_chars, (bytes, bytearray)) else np.ascontiguousarray(read_chars, dtype=np.uint8)
    t = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    o = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    ends = None if sequence_ends is None else np.ascontiguousarray(sequence_ends, dtype=np.uint64)
    n = max(o.size - 1, 0)
    arrays = {name: np.ascontiguousarray(slots[name], dtype=dtype) for name, dtype in VERIFY_SLOT_INPUTS}
    shape = arrays["sequences"].shape
    if len(shape) != 2 or shape[0] != n or any(a.shape != shape for a in arrays.values()):
        raise ValueError("the slot arrays are shaped (reads, max_candidates)")
    names = [name for name, _ in SCORE_SLOT_OUTPUTS + SCORE_READ_OUTPUTS] + ["numUnscored", "numMapped"]
    outputs = names if outputs is None else list(outputs)
    result = {name: np.zeros(shape, dtype) for name, dtype in SCORE_SLOT_OUTPUTS if name in outputs}
    result.update({name: np.zeros(n, dtype) for name, dtype in SCORE_READ_OUTPUTS if name in outputs})
    for a in result.values():
        if fill is not None:
            a.view(np.uint8)[...] = fill
    counters = {"numUnscored": np.array([unscored_before], np.uint64), "numMapped": np.array([mapped_before], np.uint64)}
    dummy = np.zeros(1, np.uint64)  # what an empty array points to: alive until the call has returned

    def address(a):
        return a.ctypes.data if a is not None and a.size else dummy.ctypes.data

    vin = verify_inputs(address(chars), chars.size if num_read_chars is None else num_read_chars, address(o),
                        **{name: address(a) for name, a in arrays.items()})
    sout = slot_score_outputs(**{name: address(a) for name, a in result.items()})
    for name, counter in counters.items():
        if name in outputs:
            setattr(sout, name, counter.ctypes.data)
    rc = getattr(_lib.lib(), symbol)(C.byref(vin), n, shape[1], band_pad, max_drift, None if costs is None else C.byref(costs), *behind,
                                     min_score, mapq_cap, address(t), t.size, None if ends is None or not ends.size else ends.ctypes.data,
                                     0 if ends is None else ends.size, alphabet, C.byref(sout), threads)
    _check(symbol, rc)
    for name, counter in counters.items():
        if name in outputs:
            result[name] = int(counter[0])
    return result


WINDOW_MAX_WIDTH = 4096   # AWFM_WINDOW_MAX_WIDTH: text characters per window after clipping to the record
WINDOW_MAX_LENGTH = 4096  # AWFM_WINDOW_MAX_LENGTH: read characters
WINDOW_READ_OUTPUTS = (("scores", np.uint32), ("readBegins", np.uint32), ("readEnds", np.uint32), ("textBegins", np.uint64),
                       ("textEnds", np.uint64))


def window_inputs(read_chars, num_read_chars, read_offsets, window_sequences, window_begins, window_ends):
    """struct AwFmWindowInputs from addresses: the read buffer, its size, the read offsets and the three per-read window arrays"""
    return _lib.AwFmWindowInputs(read_chars or None, num_read_chars, read_offsets or None, window_sequences or None, window_begins or None,
                                 window_ends or None)


def window_score_outputs(**addresses):
    """struct AwFmWindowOutputs from addresses by field name (scores, readBegins, readEnds, textBegins, textEnds, the six slot arrays
    sequences, chainAnchors, chainReadBegins, chainReadEnds, chainBeginDiagonals, chainEndDiagonals, numUnscored, numFound); a field
    left out is NULL"""
    out = _lib.AwFmWindowOutputs()
    for name, address in addresses.items():
        if name not in dict(_lib.AwFmWindowOutputs._fields_):
            raise ValueError(f"no output called {name}")
        setattr(out, name, address or None)
    return out


def score_windows_affine(read_chars, read_offsets, window_sequences, window_begins, window_ends, text, sequence_ends=None,
                         alphabet=AwFmAlphabetDna, scoring=AFFINE_SCORING, min_score=0, slots=None, slot_stride=1, slot_column=0, threads=4,
                         outputs=None, num_read_chars=None, fill=None, unscored_before=0, found_before=0):
    """awfmScoreWindowsAffine (include/awfm_gpu.h, "window scores"), the host twin: the full-width local affine alignment of read r
    against the window [window_begins[r], window_ends[r]) of record window_sequences[r] -> a dict of scores, readBegins, readEnds,
    textBegins, textEnds per read, the six slot arrays shaped (reads, slot_stride) of which column slot_column is written,
    numUnscored and numFound (ints: the values before plus this call's).  slots: a dict of slot arrays to write into (copied;
    None: arrays of the unused slot), so that the reads not looked at keep theirs.  outputs: the names to compute (None: all);
    the others are passed as NULL and left out.  fill: the value (per byte) the per-read arrays hold before the call."""
    chars = np.frombuffer(read_chars, np.uint8) if isinstance(read_chars, (bytes, bytearray)) else np.ascontiguousarray(read_chars, dtype=np.uint8)
    t = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    o = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    ends = None if sequence_ends is None else np.ascontiguousarray(sequence_ends, dtype=np.uint64)
    n = max(o.size - 1, 0)
    ws = np.ascontiguousarray(window_sequences, dtype=np.uint32)
    wb = np.ascontiguousarray(window_begins, dtype=np.uint64)
    we = np.ascontiguousarray(window_ends, dtype=np.uint64)
    if ws.shape != (n,) or wb.shape != (n,) or we.shape != (n,):
        raise ValueError("the window arrays are shaped (reads,)")
    names = [name for name, _ in WINDOW_READ_OUTPUTS] + [name for name, _ in VERIFY_SLOT_INPUTS] + ["numUnscored", "numFound"]
    outputs = names if outputs is None else list(outputs)
    result = {name: np.zeros(n, dtype) for name, dtype in WINDOW_READ_OUTPUTS if name in outputs}
    for a in result.values():
        if fill is not None:
            a.view(np.uint8)[...] = fill
    rows = max(n, 1) if not 1 <= slot_stride <= 16 else n  # (a refused stride never indexes the arrays)
    for name, dtype in VERIFY_SLOT_INPUTS:
        if name in outputs:
            if slots is not None:
                result[name] = np.array(slots[name], dtype=dtype, order="C")
            else:
                result[name] = np.zeros((rows, max(min(int(slot_stride), 16), 1)), dtype)
                if name == "sequences":
                    result[name][...] = 0xFFFFFFFF
    counters = {"numUnscored": np.array([unscored_before], np.uint64), "numFound": np.array([found_before], np.uint64)}
    dummy = np.zeros(1, np.uint64)  # what an empty array points to: alive until the call has returned

    def address(a):
        return a.ctypes.data if a is not None and a.size else dummy.ctypes.data

    win = window_inputs(address(chars), chars.size if num_read_chars is None else num_read_chars, address(o), address(ws), address(wb), address(we))
    wout = window_score_outputs(**{name: address(a) for name, a in result.items()})
    for name, counter in counters.items():
        if name in outputs:
            setattr(wout, name, counter.ctypes.data)
    costs = scoring if isinstance(scoring, _lib.AwFmAlignScoring) else align_scoring(*scoring)
    rc = _lib.lib().awfmScoreWindowsAffine(C.byref(win), n, C.byref(costs), min_score, slot_stride, slot_column, address(t), t.size,
                                           None if ends is None or not ends.size else ends.ctypes.data, 0 if ends is None else ends.size,
                                           alphabet, C.byref(wout), threads)
    _check("awfmScoreWindowsAffine", rc)
    for name, counter in counters.items():
        if name in outputs:
            result[name] = int(counter[0])
    return result


COMPLEMENT_ALL, COMPLEMENT_ODD, COMPLEMENT_EVEN = 0, 1, 2  # AWFM_COMPLEMENT_*: the reads reverse_complement_reads selects
PAIR_MAX_INSERT = 1 << 40  # AWFM_PAIR_MAX_INSERT: |min_insert|, |max_insert| <= this
PAIR_SLOT_INPUTS = (("sequences", np.uint32), ("slotScores", np.uint32), ("slotReadEnds", np.uint32), ("slotTextEnds", np.uint64))
PAIR_PAIR_OUTPUTS = (("properPairs", np.uint8), ("pairScores", np.uint32), ("pairSecondScores", np.uint32), ("templateLengths", np.int64),
                     ("pairQualities", np.uint8))
PAIR_READ_OUTPUTS = (("pairSlots", np.uint32), ("mappingQualities", np.uint8), ("windowSequences", np.uint32), ("windowBegins", np.uint64),
                     ("windowEnds", np.uint64))


def pair_inputs(read_offsets, sequences, slot_scores, slot_read_ends, slot_text_ends, mapping_qualities=0):
    """struct AwFmPairInputs from addresses: the read offsets, the slot table's sequences, the three per-slot arrays slot scores
    wrote and (0: NULL, every quality 0) its mapping qualities"""
    return _lib.AwFmPairInputs(read_offsets or None, sequences or None, slot_scores or None, slot_read_ends or None, slot_text_ends or None,
                               mapping_qualities or None)


def pair_params(min_insert, max_insert, min_score=0, unpaired_penalty=0, window_pad=0, mapq_cap=60):
    """struct AwFmPairParams"""
    return _lib.AwFmPairParams(min_insert, max_insert, min_score, unpaired_penalty, window_pad, mapq_cap)


def pair_outputs(**addresses):
    """struct AwFmPairOutputs from addresses by field name (properPairs, pairSlots, pairScores, pairSecondScores, templateLengths,
    pairQualities, mappingQualities, windowSequences, windowBegins, windowEnds, numProper, numWindows); a field left out is NULL"""
    out = _lib.AwFmPairOutputs()
    for name, address in addresses.items():
        if name not in dict(_lib.AwFmPairOutputs._fields_):
            raise ValueError(f"no output called {name}")
        setattr(out, name, address or None)
    return out


def pair_mates_host(read_offsets, slots, min_insert, max_insert, mapping_qualities=None, min_score=0, unpaired_penalty=0, window_pad=0,
                    mapq_cap=60, threads=4, outputs=None, fill=None, proper_before=0, windows_before=0, max_candidates=None):
    """awfmPairMates (include/awfm_gpu.h, "pair mates"), the host twin: reads 2p and 2p + 1 are a pair on one strand; slots: a dict
    of sequences, slotScores, slotReadEnds, slotTextEnds shaped (reads, max_candidates) as score_chains_affine_host returns them
    -> a dict of properPairs, pairScores, pairSecondScores, templateLengths, pairQualities per pair, pairSlots, mappingQualities,
    windowSequences, windowBegins, windowEnds per read, numProper and numWindows (ints: the values before plus this call's).
    outputs: the names to compute (None: all); the others are passed as NULL and left out.  fill: the value (per byte) the arrays
    hold before the call.  max_candidates: what the call is told (None: the arrays' second dimension)."""
    o = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    n = max(o.size - 1, 0)
    if n % 2:
        raise ValueError("pairs are reads 2p and 2p + 1: an even number of reads")
    arrays = {name: np.ascontiguousarray(slots[name], dtype=dtype) for name, dtype in PAIR_SLOT_INPUTS}
    shape = arrays["sequences"].shape
    if len(shape) != 2 or shape[0] != n or any(a.shape != shape for a in arrays.values()):
        raise ValueError("the slot arrays are shaped (reads, max_candidates)")
    given = None if mapping_qualities is None else np.ascontiguousarray(mapping_qualities, dtype=np.uint8)
    if given is not None and given.shape != (n,):
        raise ValueError("mapping_qualities is shaped (reads,)")
    names = [name for name, _ in PAIR_PAIR_OUTPUTS + PAIR_READ_OUTPUTS] + ["numProper", "numWindows"]
    outputs = names if outputs is None else list(outputs)
    result = {name: np.zeros(n // 2, dtype) for name, dtype in PAIR_PAIR_OUTPUTS if name in outputs}
    result.update({name: np.zeros(n, dtype) for name, dtype in PAIR_READ_OUTPUTS if name in outputs})
    for a in result.values():
        if fill is not None:
            a.view(np.uint8)[...] = fill
    counters = {"numProper": np.array([proper_before], np.uint64), "numWindows": np.array([windows_before], np.uint64)}
    dummy = np.zeros(1, np.uint64)  # what an empty array points to: alive until the call has returned

    def address(a):
        return a.ctypes.data if a is not None and a.size else dummy.ctypes.data

    pin = pair_inputs(address(o), *(address(arrays[name]) for name, _ in PAIR_SLOT_INPUTS), 0 if given is None else address(given))
    pout = pair_outputs(**{name: address(a) for name, a in result.items()})
    for name, counter in counters.items():
        if name in outputs:
            setattr(pout, name, counter.ctypes.data)
    params = pair_params(min_insert, max_insert, min_score, unpaired_penalty, window_pad, mapq_cap)
    rc = _lib.lib().awfmPairMates(C.byref(pin), n // 2, shape[1] if max_candidates is None else max_candidates, C.byref(params), C.byref(pout),
                                  threads)
    _check("awfmPairMates", rc)
    for name, counter in counters.items():
        if name in outputs:
            result[name] = int(counter[0])
    return result


def reverse_complement_reads_host(read_chars, read_offsets, which=COMPLEMENT_ODD, threads=4, num_read_chars=None, fill=0,
                                  malformed_before=0):
    """awfmReverseComplementReads (include/awfm_gpu.h, "pair mates"), DNA: -> (out uint8[len(read_chars)], numMalformed): the reads
    `which` selects (COMPLEMENT_ALL, COMPLEMENT_ODD: mate 2 of interleaved pairs, COMPLEMENT_EVEN) reverse-complemented, the others
    copied, a malformed read neither read nor written and counted.  fill: what the output holds before the call."""
    chars = np.frombuffer(read_chars, np.uint8) if isinstance(read_chars, (bytes, bytearray)) else np.ascontiguousarray(read_chars, dtype=np.uint8)
    o = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    n = max(o.size - 1, 0)
    out = np.full(chars.size, fill, np.uint8)
    counter = np.array([malformed_before], np.uint64)
    dummy = np.zeros(1, np.uint64)
    rc = _lib.lib().awfmReverseComplementReads(chars.ctypes.data if chars.size else dummy.ctypes.data,
                                               chars.size if num_read_chars is None else num_read_chars,
                                               o.ctypes.data if o.size else dummy.ctypes.data, n, which,
                                               out.ctypes.data if out.size else dummy.ctypes.data + 4, counter.ctypes.data, threads)
    _check("awfmReverseComplementReads", rc)
    return out, int(counter[0])


STRANDS_PAIRED = 1  # AWFM_STRANDS_PAIRED: reads 2p and 2p + 1 are mates from opposite strands
STRAND_READ_OUTPUTS = (("strands", np.uint8), ("strandSlots", np.uint32), ("bestScores", np.uint32), ("secondScores", np.uint32),
                       ("mappingQualities", np.uint8), ("baseFlags", np.uint16))
STRAND_ROW_OUTPUTS = (("rowSlots", np.uint32), ("windowSequences", np.uint32), ("windowBegins", np.uint64), ("windowEnds", np.uint64))
STRAND_PAIR_OUTPUTS = PAIR_PAIR_OUTPUTS
STRAND_COUNTERS = ("numReverse", "numProper", "numWindows", "numMalformed")
ORIENT_SCORE_COLUMNS = (("slotScores", np.uint32), ("slotReadEnds", np.uint32), ("slotTextEnds", np.uint64))


def strand_inputs(read_offsets, sequences, slot_scores, slot_read_ends, slot_text_ends):
    """struct AwFmStrandInputs from addresses: the offsets of the 2R rows, the slot table's sequences and the three per-slot arrays
    slot scores wrote"""
    return _lib.AwFmStrandInputs(read_offsets or None, sequences or None, slot_scores or None, slot_read_ends or None, slot_text_ends or None)


def strand_outputs(**addresses):
    """struct AwFmStrandOutputs from addresses by field name (strands, strandSlots, bestScores, secondScores, mappingQualities,
    baseFlags per read; rowSlots, windowSequences, windowBegins, windowEnds per row; properPairs, pairScores, pairSecondScores,
    templateLengths, pairQualities per pair; numReverse, numProper, numWindows, numMalformed); a field left out is NULL"""
    out = _lib.AwFmStrandOutputs()
    for name, address in addresses.items():
        if name not in dict(_lib.AwFmStrandOutputs._fields_):
            raise ValueError(f"no output called {name}")
        setattr(out, name, address or None)
    return out


def orient_inputs(rows, strands, qualities=0, **score_addresses):
    """struct AwFmOrientInputs from addresses: rows, a verify_inputs(...) of the 2R rows (slot columns left out are NULL), strands
    [R], the qualities parallel to the read buffer (0: NULL) and slotScores, slotReadEnds, slotTextEnds by field name"""
    oin = _lib.AwFmOrientInputs()
    oin.rows = rows
    oin.strands = strands or None
    oin.qualities = qualities or None
    for name, address in score_addresses.items():
        if name not in dict(ORIENT_SCORE_COLUMNS):
            raise ValueError(f"no score column called {name}")
        setattr(oin, name, address or None)
    return oin


def orient_outputs(read_chars, capacity, read_offsets, **addresses):
    """struct AwFmOrientOutputs from addresses: the output read buffer, its capacity, readOffsets [R + 1], and by field name
    qualities, the six slot columns, the three score columns and numMalformed; a field left out is NULL"""
    out = _lib.AwFmOrientOutputs(read_chars or None, capacity, read_offsets or None)
    for name, address in addresses.items():
        if name not in dict(_lib.AwFmOrientOutputs._fields_) or name in ("readChars", "capacity", "readOffsets"):
            raise ValueError(f"no output called {name}")
        setattr(out, name, address or None)
    return out


def choose_strands_host(read_offsets, slots, paired=False, min_insert=0, max_insert=0, min_score=0, unpaired_penalty=0, window_pad=0,
                        mapq_cap=60, threads=4, outputs=None, fill=None, before=None, max_candidates=None, flags=None):
    """awfmChooseStrands (include/awfm_gpu.h, "strands"), the host twin: read_offsets [2R + 1] of the rows -- the reads as
    sequenced, then their reverse complements --; slots: a dict of sequences, slotScores, slotReadEnds, slotTextEnds shaped (2R,
    max_candidates) as the slot score calls return them on the 2R rows -> a dict of strands, strandSlots, bestScores, secondScores,
    mappingQualities, baseFlags per read, rowSlots, windowSequences, windowBegins, windowEnds per row, (paired only) properPairs,
    pairScores, pairSecondScores, templateLengths, pairQualities per pair, and the counters numReverse, numProper, numWindows,
    numMalformed (ints: the values `before`, a dict, plus this call's).  outputs: the names to compute (None: all); the others are
    passed as NULL and left out.  fill: the value (per byte) the arrays hold before the call.  flags: what the call is told
    instead of `paired`."""
    o = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    rows = max(o.size - 1, 0)
    if rows % 2:
        raise ValueError("the rows are the reads and their reverse complements: an even number")
    n = rows // 2
    arrays = {name: np.ascontiguousarray(slots[name], dtype=dtype) for name, dtype in PAIR_SLOT_INPUTS}
    shape = arrays["sequences"].shape
    if len(shape) != 2 or shape[0] != rows or any(a.shape != shape for a in arrays.values()):
        raise ValueError("the slot arrays are shaped (rows, max_candidates)")
    pair_outputs_ = STRAND_PAIR_OUTPUTS if paired else ()
    names = [name for name, _ in STRAND_READ_OUTPUTS + STRAND_ROW_OUTPUTS + pair_outputs_] + list(STRAND_COUNTERS)
    outputs = names if outputs is None else list(outputs)
    result = {name: np.zeros(n, dtype) for name, dtype in STRAND_READ_OUTPUTS if name in outputs}
    result.update({name: np.zeros(rows, dtype) for name, dtype in STRAND_ROW_OUTPUTS if name in outputs})
    result.update({name: np.zeros(n // 2, dtype) for name, dtype in pair_outputs_ if name in outputs})
    for a in result.values():
        if fill is not None:
            a.view(np.uint8)[...] = fill
    counters = {name: np.array([(before or {}).get(name, 0)], np.uint64) for name in STRAND_COUNTERS}
    dummy = np.zeros(1, np.uint64)  # what an empty array points to: alive until the call has returned

    def address(a):
        return a.ctypes.data if a.size else dummy.ctypes.data

    sin = strand_inputs(address(o), *(address(arrays[name]) for name, _ in PAIR_SLOT_INPUTS))
    sout = strand_outputs(**{name: address(a) for name, a in result.items()})
    for name, counter in counters.items():
        if name in outputs:
            setattr(sout, name, counter.ctypes.data)
    params = pair_params(min_insert, max_insert, min_score, unpaired_penalty, window_pad, mapq_cap)
    rc = _lib.lib().awfmChooseStrands(C.byref(sin), n, shape[1] if max_candidates is None else max_candidates,
                                      (STRANDS_PAIRED if paired else 0) if flags is None else flags, C.byref(params), C.byref(sout), threads)
    _check("awfmChooseStrands", rc)
    for name, counter in counters.items():
        if name in outputs:
            result[name] = int(counter[0])
    return result


def orient_reads_host(read_chars, read_offsets, strands, slots=None, qualities=None, capacity=None, threads=4, fill=0, malformed_before=0,
                      num_read_chars=None, max_candidates=None):
    """awfmOrientReads (include/awfm_gpu.h, "strands"), the host twin: read_chars and read_offsets [2R + 1] of the 2R rows, strands
    [R]; slots: a dict of any of the six slot columns and slotScores, slotReadEnds, slotTextEnds, shaped (2R, max_candidates);
    qualities parallel to read_chars -> a dict of readChars (uint8[capacity]; None: what the reads need), readOffsets [R + 1],
    qualities and the given columns shaped (R, max_candidates), and numMalformed.  fill: what the outputs hold before the call."""
    chars = np.frombuffer(read_chars, np.uint8) if isinstance(read_chars, (bytes, bytearray)) else np.ascontiguousarray(read_chars, dtype=np.uint8)
    o = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    rows = max(o.size - 1, 0)
    if rows % 2:
        raise ValueError("the rows are the reads and their reverse complements: an even number")
    n = rows // 2
    s = np.ascontiguousarray(strands, dtype=np.uint8)
    if s.shape != (n,):
        raise ValueError("strands is shaped (reads,)")
    quals = None if qualities is None else np.ascontiguousarray(qualities, dtype=np.uint8)
    if capacity is None:
        capacity = int(o[n] - o[0]) if n and o[n] >= o[0] else 0
    dtypes = dict(VERIFY_SLOT_INPUTS + ORIENT_SCORE_COLUMNS)
    columns = {name: np.ascontiguousarray(a, dtype=dtypes[name]) for name, a in (slots or {}).items()}
    widths = {a.shape[1] for a in columns.values() if a.ndim == 2}
    if any(a.ndim != 2 or a.shape[0] != rows for a in columns.values()) or len(widths) > 1:
        raise ValueError("the slot columns are shaped (rows, max_candidates)")
    width = max_candidates if max_candidates is not None else widths.pop() if widths else 1
    result = {"readChars": np.full(capacity, fill, np.uint8), "readOffsets": np.zeros(n + 1, np.uint64)}
    if quals is not None:
        result["qualities"] = np.full(capacity, fill, np.uint8)
    for name, a in columns.items():
        result[name] = np.zeros((n, width), a.dtype)
        result[name].view(np.uint8)[...] = fill
    counter = np.array([malformed_before], np.uint64)
    dummy = np.zeros(2, np.uint64)

    def address(a):
        return a.ctypes.data if a.size else dummy.ctypes.data

    rows_in = verify_inputs(address(chars), chars.size if num_read_chars is None else num_read_chars, address(o),
                            **{name: address(a) for name, a in columns.items() if name in dict(VERIFY_SLOT_INPUTS)})
    oin = orient_inputs(rows_in, address(s), 0 if quals is None else address(quals),
                        **{name: address(a) for name, a in columns.items() if name in dict(ORIENT_SCORE_COLUMNS)})
    oout = orient_outputs(result["readChars"].ctypes.data if capacity else dummy.ctypes.data + 8, capacity, address(result["readOffsets"]),
                          numMalformed=counter.ctypes.data,
                          **{name: (a.ctypes.data if a.size else dummy.ctypes.data + 8) for name, a in result.items()
                             if name not in ("readChars", "readOffsets")})
    _check("awfmOrientReads", _lib.lib().awfmOrientReads(C.byref(oin), n, width, C.byref(oout), threads))
    result["numMalformed"] = int(counter[0])
    return result


INSERT_MAX_BINS, INSERT_MAX_SPREAD = 65536, 16  # AWFM_INSERT_MAX_BINS, AWFM_INSERT_MAX_SPREAD
INSERT_ESTIMATE_FIELDS = ("minInsert", "maxInsert", "quartiles", "mean", "numSamples", "valid")


def insert_params(low_template, high_template, min_score=0, min_quality=0, spread=2, min_samples=16, fallback_min=0, fallback_max=1000):
    """struct AwFmInsertParams (include/awfm_gpu.h, "insert size"): the histogram's range [low_template, high_template], who
    qualifies (min_score, min_quality), the interval's spread in interquartile ranges and the fallback interval of a histogram
    with fewer than min_samples samples"""
    return _lib.AwFmInsertParams(low_template, high_template, min_score, min_quality, spread, min_samples, fallback_min, fallback_max)


def insert_estimate_dict(estimate):
    """struct AwFmInsertEstimate (or its 64 bytes as an array) -> a dict of Python integers, quartiles a list of three"""
    if not isinstance(estimate, _lib.AwFmInsertEstimate):
        estimate = _lib.AwFmInsertEstimate.from_buffer_copy(np.ascontiguousarray(estimate).tobytes())
    return dict(minInsert=int(estimate.minInsert), maxInsert=int(estimate.maxInsert), quartiles=[int(q) for q in estimate.quartiles],
                mean=int(estimate.mean), numSamples=int(estimate.numSamples), valid=int(estimate.valid))


def insert_histogram_host(read_offsets, slots, params, mapping_qualities=None, histogram=None, samples_before=0, outside_before=0, threads=4,
                          counters=("numSamples", "numOutside"), max_candidates=None):
    """awfmInsertHistogram (include/awfm_gpu.h, "insert size"), the host twin: slots as pair_mates_host takes them, params an
    insert_params(...) -> (histogram uint64[bins], numSamples, numOutside).  The histogram is ADDED TO: `histogram` (None: zeros)
    is what it holds before the call and is not changed itself; so are the counters, which start from samples_before and
    outside_before; a counter not named in `counters` is passed as NULL and comes back as None."""
    o = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    n = max(o.size - 1, 0)
    if n % 2:
        raise ValueError("pairs are reads 2p and 2p + 1: an even number of reads")
    arrays = {name: np.ascontiguousarray(slots[name], dtype=dtype) for name, dtype in PAIR_SLOT_INPUTS}
    shape = arrays["sequences"].shape
    if len(shape) != 2 or shape[0] != n or any(a.shape != shape for a in arrays.values()):
        raise ValueError("the slot arrays are shaped (reads, max_candidates)")
    given = None if mapping_qualities is None else np.ascontiguousarray(mapping_qualities, dtype=np.uint8)
    if given is not None and given.shape != (n,):
        raise ValueError("mapping_qualities is shaped (reads,)")
    bins = max(min(int(params.highTemplate) - int(params.lowTemplate) + 1, INSERT_MAX_BINS), 1)
    result = np.zeros(bins, np.uint64) if histogram is None else np.array(histogram, dtype=np.uint64)
    if result.shape != (bins,):
        raise ValueError("the histogram has highTemplate - lowTemplate + 1 bins")
    samples, outside = np.array([samples_before], np.uint64), np.array([outside_before], np.uint64)
    dummy = np.zeros(1, np.uint64)  # what an empty array points to: alive until the call has returned

    def address(a):
        return a.ctypes.data if a is not None and a.size else dummy.ctypes.data

    pin = pair_inputs(address(o), *(address(arrays[name]) for name, _ in PAIR_SLOT_INPUTS), 0 if given is None else address(given))
    rc = _lib.lib().awfmInsertHistogram(C.byref(pin), n // 2, shape[1] if max_candidates is None else max_candidates, C.byref(params),
                                        result.ctypes.data, samples.ctypes.data if "numSamples" in counters else None,
                                        outside.ctypes.data if "numOutside" in counters else None, threads)
    _check("awfmInsertHistogram", rc)
    return result, int(samples[0]) if "numSamples" in counters else None, int(outside[0]) if "numOutside" in counters else None


def insert_interval_host(histogram, params):
    """awfmInsertInterval (include/awfm_gpu.h, "insert size"), the host twin: the histogram's quartiles -> a dict of minInsert,
    maxInsert, quartiles (three), mean, numSamples, valid (0: the fallback interval)"""
    h = np.ascontiguousarray(histogram, dtype=np.uint64)
    estimate = _lib.AwFmInsertEstimate()
    _check("awfmInsertInterval", _lib.lib().awfmInsertInterval(h.ctypes.data if h.size else None, C.byref(params), C.byref(estimate)))
    return insert_estimate_dict(estimate)


def estimate_insert_size_host(read_offsets, slots, params, mapping_qualities=None, threads=4):
    """insert_histogram_host on a histogram of zeros, then insert_interval_host -> the interval's dict with histogram,
    numOutside added"""
    histogram, _, outside = insert_histogram_host(read_offsets, slots, params, mapping_qualities=mapping_qualities, threads=threads)
    return dict(insert_interval_host(histogram, params), histogram=histogram, numOutside=outside)


AWFM_EDIT_NONE = 0xFFFFFFFF  # the edit of a record of the unedited query (include/awfm_gpu.h)


def one_substitution_search_host(index, chars, offsets=None, fixed_length=0, include_exact=True, capacity=None, threads=4):
    """awfmOneSubstitutionSearch: for query i = chars[offsets[i]:offsets[i + 1]] (offsets None: fixed_length characters per
    query) one record per string at Hamming distance 1 that occurs in the text (edit = position * 32 + letter index), and with
    include_exact one for the query itself (edit AWFM_EDIT_NONE) -> (queries uint32[k], edits uint32[k], ranges uint64[k, 2],
    num_hits, variants uint32[n], occurrences uint64[n]), sorted by (query, edit).  capacity None: counts first, then fills
    (k = num_hits); otherwise k = min(capacity, num_hits), num_hits stays the true number, the per-query arrays are complete."""
    chars = np.ascontiguousarray(np.frombuffer(chars, np.uint8) if isinstance(chars, (bytes, bytearray)) else chars, dtype=np.uint8)
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.size - 1, 0)
    else:
        if fixed_length <= 0:
            raise ValueError("queries need offsets or a fixed length")
        n = chars.size // fixed_length
    variants = np.zeros(n, np.uint32)
    occurrences = np.zeros(n, np.uint64)
    holder = chars if chars.size else np.zeros(1, np.uint8)
    total = C.c_uint64(0)

    def call(queries, edits, ranges, cap):
        rc = _lib.lib().awfmOneSubstitutionSearch(index.ptr, holder.ctypes.data, offsets.ctypes.data if offsets is not None and n else None,
                                                  fixed_length, n, 1 if include_exact else 0,
                                                  queries.ctypes.data if cap else None, edits.ctypes.data if cap else None,
                                                  ranges.ctypes.data if cap else None, cap, C.byref(total),
                                                  variants.ctypes.data if n else None, occurrences.ctypes.data if n else None, threads)
        _check("awfmOneSubstitutionSearch", rc)

    if capacity is None:
        call(None, None, None, 0)
        capacity = int(total.value)
    queries = np.zeros(capacity, np.uint32)
    edits = np.zeros(capacity, np.uint32)
    ranges = np.zeros((capacity, 2), np.uint64)
    call(queries, edits, ranges, capacity)
    k = min(capacity, int(total.value))
    return queries[:k], edits[:k], ranges[:k], int(total.value), variants, occurrences


# enum AwFmGpuKernel (include/awfm_gpu.h)
AWFM_GPU_KERNEL_AUTO, AWFM_GPU_KERNEL_GROUP8, AWFM_GPU_KERNEL_GROUP4, AWFM_GPU_KERNEL_GROUP2, AWFM_GPU_KERNEL_GROUP1 = range(5)


class GpuIndex:
    """AwFmGpuIndex* owner: the device image plus the flat batch API of include/awfm_gpu.h"""

    def __init__(self, index, device=-1, acquire=False):
        """acquire=True reuses (or lazily creates) the image registered for `index` -- the one
        awFmParallelSearch* uses, e.g. the image a GPU-built index already has; it is then owned by the index"""
        L = _lib.lib()
        if L.awfmGpuDeviceCount() <= 0:
            raise RuntimeError("no HIP device: the search path is GPU only (no CPU fallback)")
        self.owned = not acquire
        if acquire:
            h = L.awfmGpuIndexAcquire(index.ptr)
            if not h:
                raise AwFmError("awfmGpuIndexAcquire", -1)
            self.handle = C.c_void_p(h)
        else:
            h = C.c_void_p()
            _check("awfmGpuIndexCreate", L.awfmGpuIndexCreate(index.ptr, device, C.byref(h)))
            self.handle = h
        self.index = index

    @classmethod
    def acquire_all(cls, index, max_handles=8):
        """awfmGpuIndexAcquireAll: the handles awFmParallelSearch* deal their chunks to ($AWFM_GPU_DEVICES; unset: three
        lanes on one image of the default device), owned by the index"""
        L = _lib.lib()
        if L.awfmGpuDeviceCount() <= 0:
            raise RuntimeError("no HIP device: the search path is GPU only (no CPU fallback)")
        handles = (C.c_void_p * max_handles)()
        n = L.awfmGpuIndexAcquireAll(index.ptr, handles, max_handles)
        out = []
        for h in handles[:n]:
            g = cls.__new__(cls)
            g.owned, g.handle, g.index = False, C.c_void_p(h), index
            out.append(g)
        return out

    @property
    def device_bytes(self):
        return int(_lib.lib().awfmGpuIndexDeviceBytes(self.handle))

    def set_deep_seed(self, deep_k):
        """device-only deeper seed table (nucleotide); 0 drops it"""
        _check("awfmGpuIndexSetDeepSeed", _lib.lib().awfmGpuIndexSetDeepSeed(self.handle, deep_k))

    @property
    def deep_seed_k(self):
        """depth of the device-only deeper seed table of this image (0: none)"""
        return int(_lib.lib().awfmGpuIndexDeepSeedK(self.handle))

    @property
    def deep_seed_build(self):
        """(wall seconds, transient device bytes) of the construction of that table, whoever started it"""
        L = _lib.lib()
        return float(L.awfmGpuIndexDeepSeedBuildSeconds(self.handle)), int(L.awfmGpuIndexDeepSeedTransientBytes(self.handle))

    @property
    def deep_seed_alloc_s(self):
        """seconds of that construction spent inside hipMalloc"""
        return float(_lib.lib().awfmGpuIndexDeepSeedAllocSeconds(self.handle))

    def set_dense_sa(self, enable=True):
        """device-only full suffix array (32-bit entries) so that a locate is a single gather"""
        _check("awfmGpuIndexSetDenseSa", _lib.lib().awfmGpuIndexSetDenseSa(self.handle, int(bool(enable))))

    @property
    def has_dense_sa(self):
        return bool(_lib.lib().awfmGpuIndexHasDenseSa(self.handle))

    @property
    def dense_sa_build_s(self):
        return float(_lib.lib().awfmGpuIndexDenseSaBuildSeconds(self.handle))

    @property
    def length_tables(self):
        """(bytes, build seconds) of the device-only tables per k-mer length a mixed-length batch builds on first use; (0, 0.0): none"""
        return (int(_lib.lib().awfmGpuIndexLengthTableBytes(self.handle)), float(_lib.lib().awfmGpuIndexLengthTableBuildSeconds(self.handle)))

    def mixed_lookup_line_tally(self, d_chars, d_offsets, n):
        """what the lookup-first kernel of mixed-length batches has to read for this batch (awfmGpuMixedLookupLineTally)"""
        out = (C.c_uint64 * 8)()
        _check("awfmGpuMixedLookupLineTally", _lib.lib().awfmGpuMixedLookupLineTally(self.handle, d_chars, d_offsets, n, C.byref(out)))
        keys = ("length_table_lines", "deep_table_lines", "pair_level_lines", "nuc_level_lines", "kmers_alive_after_the_table",
                "kmers_with_hits", "general_kmers", "block_reads_executed")
        return {k: int(v) for k, v in zip(keys, out)}

    def set_pair_image(self, enable=True):
        """device-only pair image (two steps per block read); built by default with nucleotide images"""
        _check("awfmGpuIndexSetPairImage", _lib.lib().awfmGpuIndexSetPairImage(self.handle, int(bool(enable))))

    @property
    def has_pair_image(self):
        return bool(_lib.lib().awfmGpuIndexHasPairImage(self.handle))

    def set_kernel(self, kernel):
        """enum AwFmGpuKernel (include/awfm_gpu.h): AWFM_GPU_KERNEL_AUTO, or a fixed number of lanes per k-mer for the general
        kernel and the walk -- anything but AUTO / GROUP4 keeps a search away from the pair image and the device-only tables,
        i.e. runs the reference's letter-by-letter algorithm (what the differential fuzz compares everything else with)"""
        _lib.lib().awfmGpuIndexSetKernel(self.handle, kernel)

    def set_wide(self, wide=True):
        """64-bit BWT positions in the kernels although bwtLength < 2^32 (testing)"""
        _lib.lib().awfmGpuIndexSetWide(self.handle, int(bool(wide)))

    @property
    def is_wide(self):
        return bool(_lib.lib().awfmGpuIndexIsWide(self.handle))

    # sequence coordinates (include/awfm_gpu.h) ---------------------------
    def set_record_table(self, ends):
        """awfmGpuIndexSetRecordTable: installs or replaces the image's record table from the records' ends in the concatenated
        text (terminators excluded); an empty array drops it"""
        ends = np.ascontiguousarray(ends, dtype=np.uint64)
        _check("awfmGpuIndexSetRecordTable", _lib.lib().awfmGpuIndexSetRecordTable(self.handle, ends.ctypes.data if ends.size else None,
                                                                                   ends.size))

    @property
    def num_records(self):
        """records of the image's record table (0: none)"""
        return int(_lib.lib().awfmGpuIndexNumRecords(self.handle))

    def local_positions(self, d_positions, capacity, d_seq, d_local, d_num_positions=0, d_num_illegal=0, stream=0):
        """awfmGpuLocalPositions: the first min(*d_num_positions, capacity) positions (capacity without a count) to
        (sequence number, local position) on the device; d_local may be d_positions; *d_num_illegal is added to"""
        _check("awfmGpuLocalPositions", _lib.lib().awfmGpuLocalPositions(self.handle, d_positions or None, capacity, d_num_positions or None,
                                                                         d_seq or None, d_local or None, d_num_illegal or None, stream or None))

    def read_candidates(self, inputs, num_reads, outputs, d_scratch, max_hits_per_seed=0, band=0, min_votes=1, max_candidates=4, stream=0):
        """awfmGpuReadCandidates: inputs / outputs are candidate_inputs(...) / candidate_outputs(...) of device addresses, d_scratch
        read_candidates_scratch_bytes(num_reads) bytes of device memory of this call's own; asynchronous on `stream`;
        *numOverflowed is added to"""
        _check("awfmGpuReadCandidates", _lib.lib().awfmGpuReadCandidates(
            self.handle, C.byref(inputs), num_reads, max_hits_per_seed, band, min_votes, max_candidates, C.byref(outputs),
            d_scratch or None, stream or None))

    def read_chains(self, inputs, num_reads, d_sequences, d_diagonals, d_spans, outputs, d_scratch, max_hits_per_seed=0, band=0,
                    max_candidates=4, lookback=CHAINS_MAX_LOOKBACK, gap_penalty=0, stream=0):
        """awfmGpuReadChains: inputs as for read_candidates, d_sequences / d_diagonals / d_spans the slot arrays it wrote, outputs
        chain_outputs(...) of device addresses, d_scratch read_chains_scratch_bytes(num_reads) bytes of device memory of this
        call's own; asynchronous on `stream`; *numOverflowed is added to"""
        _check("awfmGpuReadChains", _lib.lib().awfmGpuReadChains(
            self.handle, C.byref(inputs), num_reads, max_hits_per_seed, band, max_candidates, d_sequences or None, d_diagonals or None,
            d_spans or None, lookback, gap_penalty, C.byref(outputs), d_scratch or None, stream or None))

    # chain verification (include/awfm_gpu.h) -----------------------------
    def set_text(self, text):
        """awfmGpuIndexSetText: uploads the indexed text (bytes or a uint8 array of bwtLength - 1 bytes, as it was given to the
        index's constructor); None or an empty text removes it"""
        if text is None:
            t = np.zeros(0, np.uint8)
        else:
            t = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
        _check("awfmGpuIndexSetText", _lib.lib().awfmGpuIndexSetText(self.handle, t.ctypes.data if t.size else None, t.size))

    @property
    def text_length(self):
        """positions of the image's text (0: none)"""
        return int(_lib.lib().awfmGpuIndexTextLength(self.handle))

    def text_windows(self, d_positions, capacity, before, after, d_out, d_num_positions=0, stream=0):
        """awfmGpuTextWindows: window i of the first min(*d_num_positions, capacity) positions (capacity without a count) is
        d_out[i * (before + after) ..) = text[p - before, p + after), zero outside the text; asynchronous on `stream`"""
        _check("awfmGpuTextWindows", _lib.lib().awfmGpuTextWindows(self.handle, d_positions or None, capacity, d_num_positions or None,
                                                                   before, after, d_out or None, stream or None))

    def verify_chains(self, inputs, num_reads, outputs, max_candidates=4, band_pad=8, max_drift=15, stream=0):
        """awfmGpuVerifyChains: inputs / outputs are verify_inputs(...) / verify_outputs(...) of device addresses; text, record
        table and alphabet are the image's; asynchronous on `stream`; *numUnverified is added to"""
        _check("awfmGpuVerifyChains", _lib.lib().awfmGpuVerifyChains(self.handle, C.byref(inputs), num_reads, max_candidates, band_pad,
                                                                     max_drift, C.byref(outputs), stream or None))

    # chain alignment (include/awfm_gpu.h) --------------------------------
    def align_chains_scratch_bytes(self, max_rows):
        """awfmGpuAlignChainsScratchBytes: the bytes of device scratch align_chains needs for reads of up to max_rows characters"""
        return int(_lib.lib().awfmGpuAlignChainsScratchBytes(self.handle, max_rows))

    def align_chains(self, inputs, d_slots, num_reads, outputs, d_scratch, max_candidates=4, band_pad=8, max_drift=15, max_ops=32,
                     max_rows=4096, stream=0):
        """awfmGpuAlignChains: inputs verify_inputs(...) and outputs align_outputs(...) of device addresses, d_slots the slot of every
        read to align (bestSlots of read_chains or verify_chains), d_scratch align_chains_scratch_bytes(max_rows) bytes of device
        memory of this call's own, aligned to 16 bytes; asynchronous on `stream`; *numUnaligned and *numTruncated are added to"""
        _check("awfmGpuAlignChains", _lib.lib().awfmGpuAlignChains(self.handle, C.byref(inputs), d_slots or None, num_reads, max_candidates,
                                                                   band_pad, max_drift, max_ops, max_rows, C.byref(outputs),
                                                                   d_scratch or None, stream or None))

    # affine alignment (include/awfm_gpu.h) -------------------------------
    def align_chains_affine_scratch_bytes(self, max_rows):
        """awfmGpuAlignChainsAffineScratchBytes: the bytes of device scratch align_chains_affine needs for reads of up to max_rows
        characters"""
        return int(_lib.lib().awfmGpuAlignChainsAffineScratchBytes(self.handle, max_rows))

    def align_chains_affine(self, inputs, d_slots, num_reads, outputs, d_scratch, max_candidates=4, band_pad=8, max_drift=15,
                            scoring=AFFINE_SCORING, max_ops=32, max_rows=4096, stream=0):
        """awfmGpuAlignChainsAffine: inputs verify_inputs(...) and outputs affine_outputs(...) of device addresses, d_slots the slot of
        every read to align (bestSlots of read_chains or verify_chains), scoring (match, mismatch, gap_open, gap_extend) or an
        align_scoring(...), d_scratch align_chains_affine_scratch_bytes(max_rows) bytes of device memory of this call's own,
        aligned to 16 bytes; asynchronous on `stream`; *numUnaligned and *numTruncated are added to"""
        costs = None if scoring is None else scoring if isinstance(scoring, _lib.AwFmAlignScoring) else align_scoring(*scoring)
        _check("awfmGpuAlignChainsAffine",
               _lib.lib().awfmGpuAlignChainsAffine(self.handle, C.byref(inputs), d_slots or None, num_reads, max_candidates, band_pad, max_drift,
                                                   None if costs is None else C.byref(costs), max_ops, max_rows, C.byref(outputs),
                                                   d_scratch or None, stream or None))

    # substitution matrices (include/awfm_gpu.h) --------------------------
    def align_chains_matrix(self, inputs, d_slots, num_reads, outputs, d_scratch, max_candidates=4, band_pad=8, max_drift=15, scoring=None,
                            max_ops=32, max_rows=4096, stream=0):
        """awfmGpuAlignChainsMatrix: align_chains_affine with scoring a matrix_scoring(...) (None: the call's NULL); the struct may be
        changed as soon as the call returns; d_scratch is align_chains_affine_scratch_bytes(max_rows) bytes"""
        _check("awfmGpuAlignChainsMatrix",
               _lib.lib().awfmGpuAlignChainsMatrix(self.handle, C.byref(inputs), d_slots or None, num_reads, max_candidates, band_pad, max_drift,
                                                   None if scoring is None else C.byref(scoring), max_ops, max_rows, C.byref(outputs),
                                                   d_scratch or None, stream or None))

    def score_chains_matrix(self, inputs, num_reads, outputs, max_candidates=4, band_pad=8, max_drift=15, scoring=None, min_score=0,
                            mapq_cap=60, stream=0):
        """awfmGpuScoreChainsMatrix: score_chains_affine with scoring a matrix_scoring(...) (None: the call's NULL); the struct may be
        changed as soon as the call returns; one launch, no scratch"""
        _check("awfmGpuScoreChainsMatrix",
               _lib.lib().awfmGpuScoreChainsMatrix(self.handle, C.byref(inputs), num_reads, max_candidates, band_pad, max_drift,
                                                   None if scoring is None else C.byref(scoring), min_score, mapq_cap, C.byref(outputs),
                                                   stream or None))

    # end bonus (include/awfm_gpu.h) --------------------------------------
    def align_chains_end_bonus(self, inputs, d_slots, num_reads, outputs, d_scratch, max_candidates=4, band_pad=8, max_drift=15, scoring=None,
                               end_bonus=END_BONUS, max_ops=32, max_rows=4096, stream=0):
        """awfmGpuAlignChainsEndBonus: align_chains_matrix with end_bonus, 0 to 255, earned at each read end the alignment reaches;
        the scores include it; d_scratch is align_chains_affine_scratch_bytes(max_rows) bytes"""
        _check("awfmGpuAlignChainsEndBonus",
               _lib.lib().awfmGpuAlignChainsEndBonus(self.handle, C.byref(inputs), d_slots or None, num_reads, max_candidates, band_pad, max_drift,
                                                     None if scoring is None else C.byref(scoring), end_bonus, max_ops, max_rows,
                                                     C.byref(outputs), d_scratch or None, stream or None))

    def score_chains_end_bonus(self, inputs, num_reads, outputs, max_candidates=4, band_pad=8, max_drift=15, scoring=None, end_bonus=END_BONUS,
                               min_score=0, mapq_cap=60, stream=0):
        """awfmGpuScoreChainsEndBonus: score_chains_matrix with end_bonus, 0 to 255; one launch, no scratch"""
        _check("awfmGpuScoreChainsEndBonus",
               _lib.lib().awfmGpuScoreChainsEndBonus(self.handle, C.byref(inputs), num_reads, max_candidates, band_pad, max_drift,
                                                     None if scoring is None else C.byref(scoring), end_bonus, min_score, mapq_cap,
                                                     C.byref(outputs), stream or None))

    # alignment strings (include/awfm_gpu.h) ------------------------------
    def alignment_strings_scratch_bytes(self, num_reads):
        """awfmGpuAlignmentStringsScratchBytes: the bytes of device scratch alignment_strings needs for num_reads reads"""
        return int(_lib.lib().awfmGpuAlignmentStringsScratchBytes(self.handle, num_reads))

    def alignment_strings(self, inputs, num_reads, outputs, d_scratch, max_candidates=4, max_ops=32, classic=False, flags=None, stream=0):
        """awfmGpuAlignmentStrings: inputs string_inputs(...) and outputs string_outputs(...) of device addresses -- the arrays as
        align_chains or align_chains_affine left them --, d_scratch alignment_strings_scratch_bytes(num_reads) bytes of device memory
        of this call's own, aligned to 16 bytes; the CIGAR (classic: with M) and the MD:Z string of every read, packed behind
        their offsets; asynchronous on `stream`; *numSkipped and *numOverflow are added to"""
        flags = (STRINGS_CIGAR_M if classic else 0) if flags is None else flags
        _check("awfmGpuAlignmentStrings",
               _lib.lib().awfmGpuAlignmentStrings(self.handle, None if inputs is None else C.byref(inputs), num_reads, max_candidates, max_ops,
                                                  flags, None if outputs is None else C.byref(outputs), d_scratch or None, stream or None))

    # SAM records (include/awfm_gpu.h) ------------------------------------
    def sam_records_scratch_bytes(self, num_reads):
        """awfmGpuSamRecordsScratchBytes: the bytes of device scratch sam_records needs for num_reads reads"""
        return int(_lib.lib().awfmGpuSamRecordsScratchBytes(self.handle, num_reads))

    def sam_records(self, inputs, num_reads, outputs, d_scratch, max_candidates=4, paired=False, flags=None, stream=0):
        """awfmGpuSamRecords: inputs sam_inputs(...) and outputs sam_outputs(...) of device addresses -- the arrays as the alignment,
        string, score and pairing calls left them --, d_scratch sam_records_scratch_bytes(num_reads) bytes of device memory of this
        call's own, aligned to 16 bytes; one SAM line per read, packed behind lineOffsets; asynchronous on `stream`; *numUnaligned
        and *numOverflow are added to"""
        flags = (SAM_PAIRED if paired else 0) if flags is None else flags
        _check("awfmGpuSamRecords",
               _lib.lib().awfmGpuSamRecords(self.handle, None if inputs is None else C.byref(inputs), num_reads, max_candidates, flags,
                                            None if outputs is None else C.byref(outputs), d_scratch or None, stream or None))

    # slot scores and mapping quality (include/awfm_gpu.h) -----------------
    def score_chains_affine(self, inputs, num_reads, outputs, max_candidates=4, band_pad=8, max_drift=15, scoring=AFFINE_SCORING,
                            min_score=0, mapq_cap=60, stream=0):
        """awfmGpuScoreChainsAffine: inputs verify_inputs(...) and outputs slot_score_outputs(...) of device addresses, scoring (match,
        mismatch, gap_open, gap_extend) or an align_scoring(...); the affine score and end cell of every slot, per read the best
        slot (what align_chains_affine takes as d_slots), the second and the mapping quality; one launch, no scratch,
        asynchronous on `stream`; *numUnscored and *numMapped are added to"""
        costs = None if scoring is None else scoring if isinstance(scoring, _lib.AwFmAlignScoring) else align_scoring(*scoring)
        _check("awfmGpuScoreChainsAffine",
               _lib.lib().awfmGpuScoreChainsAffine(self.handle, C.byref(inputs), num_reads, max_candidates, band_pad, max_drift,
                                                   None if costs is None else C.byref(costs), min_score, mapq_cap, C.byref(outputs),
                                                   stream or None))

    # window scores (include/awfm_gpu.h) ----------------------------------
    def score_windows_affine_scratch_bytes(self, max_length):
        """awfmGpuScoreWindowsAffineScratchBytes: the bytes of device scratch score_windows_affine needs for reads of up to max_length
        characters (1..4096)"""
        return int(_lib.lib().awfmGpuScoreWindowsAffineScratchBytes(self.handle, max_length))

    def score_windows_affine(self, inputs, num_reads, outputs, d_scratch, max_length, scoring=AFFINE_SCORING, min_score=0, slot_stride=1,
                             slot_column=0, stream=0):
        """awfmGpuScoreWindowsAffine: inputs window_inputs(...) and outputs window_score_outputs(...) of device addresses, scoring
        (match, mismatch, gap_open, gap_extend) or an align_scoring(...), d_scratch score_windows_affine_scratch_bytes(max_length)
        bytes of device memory of this call's own, aligned to 16 bytes; the full-width local affine alignment of every read against
        the window it names, and column slot_column of a slot table of slot_stride columns that align_chains_affine and
        score_chains_affine take as it is; a read longer than max_length is TOO LONG; one launch, asynchronous on `stream`;
        *numUnscored and *numFound are added to"""
        costs = None if scoring is None else scoring if isinstance(scoring, _lib.AwFmAlignScoring) else align_scoring(*scoring)
        _check("awfmGpuScoreWindowsAffine",
               _lib.lib().awfmGpuScoreWindowsAffine(self.handle, C.byref(inputs), num_reads, None if costs is None else C.byref(costs), min_score,
                                                    slot_stride, slot_column, max_length, C.byref(outputs), d_scratch or None,
                                                    stream or None))

    # pair mates (include/awfm_gpu.h) --------------------------------------
    def pair_mates(self, inputs, num_pairs, outputs, min_insert, max_insert, max_candidates=4, min_score=0, unpaired_penalty=0,
                   window_pad=0, mapq_cap=60, stream=0):
        """awfmGpuPairMates: inputs pair_inputs(...) and outputs pair_outputs(...) of device addresses; reads 2p and 2p + 1 are a
        pair on one strand (reverse_complement_reads); per pair the winner among the concordant slot pairs (min_insert <= T <=
        max_insert) and the discordant candidate, the second and the pair's quality, per read pairSlots (what align_chains_affine
        takes as d_slots), the mapping quality and the rescue window (what window_inputs takes); one launch, no scratch,
        asynchronous on `stream`; *numProper and *numWindows are added to"""
        params = pair_params(min_insert, max_insert, min_score, unpaired_penalty, window_pad, mapq_cap)
        _check("awfmGpuPairMates", _lib.lib().awfmGpuPairMates(self.handle, C.byref(inputs), num_pairs, max_candidates, C.byref(params),
                                                               C.byref(outputs), stream or None))

    # insert size (include/awfm_gpu.h) --------------------------------------
    def insert_histogram(self, inputs, num_pairs, params, d_histogram, d_num_samples=0, d_num_outside=0, max_candidates=4, stream=0):
        """awfmGpuInsertHistogram: inputs pair_inputs(...) of device addresses, params insert_params(...); d_histogram, highTemplate -
        lowTemplate + 1 uint64 counters the caller zeroed, and the two counters (0: NULL) are added to; one launch, asynchronous on
        `stream`"""
        _check("awfmGpuInsertHistogram",
               _lib.lib().awfmGpuInsertHistogram(self.handle, None if inputs is None else C.byref(inputs), num_pairs, max_candidates,
                                                 None if params is None else C.byref(params), d_histogram or None, d_num_samples or None,
                                                 d_num_outside or None, stream or None))

    def insert_interval(self, d_histogram, params, d_estimate, stream=0):
        """awfmGpuInsertInterval: the 64 bytes of struct AwFmInsertEstimate at d_estimate from the histogram's quartiles (or the
        fallback); one launch of one workgroup, asynchronous on `stream`"""
        _check("awfmGpuInsertInterval", _lib.lib().awfmGpuInsertInterval(self.handle, d_histogram or None, None if params is None else C.byref(params),
                                                                        d_estimate or None, stream or None))

    def pair_mates_estimated(self, inputs, num_pairs, outputs, d_estimate, max_candidates=4, min_score=0, unpaired_penalty=0, window_pad=0,
                             mapq_cap=60, stream=0):
        """awfmGpuPairMatesEstimated: pair_mates with the interval read on the device from the struct AwFmInsertEstimate at
        d_estimate, which insert_interval wrote earlier on the stream; an interval that is not usable makes no pair proper and
        names no window"""
        params = pair_params(0, 0, min_score, unpaired_penalty, window_pad, mapq_cap)
        _check("awfmGpuPairMatesEstimated",
               _lib.lib().awfmGpuPairMatesEstimated(self.handle, C.byref(inputs), num_pairs, max_candidates, C.byref(params), d_estimate or None,
                                                    C.byref(outputs), stream or None))

    def reverse_complement_reads(self, d_read_chars, num_read_chars, d_read_offsets, num_reads, d_out, which=COMPLEMENT_ODD,
                                 d_num_malformed=0, stream=0):
        """awfmGpuReverseComplementReads (DNA): d_out, num_read_chars bytes that do not overlap the input, gets the reads `which`
        selects reverse-complemented and the others copied; one launch, asynchronous on `stream`; *d_num_malformed is added to"""
        _check("awfmGpuReverseComplementReads",
               _lib.lib().awfmGpuReverseComplementReads(self.handle, d_read_chars or None, num_read_chars, d_read_offsets or None, num_reads,
                                                        which, d_out or None, d_num_malformed or None, stream or None))

    # strands (include/awfm_gpu.h) -----------------------------------------
    def choose_strands(self, inputs, num_reads, outputs, paired=False, min_insert=0, max_insert=0, max_candidates=4, min_score=0,
                       unpaired_penalty=0, window_pad=0, mapq_cap=60, stream=0, flags=None):
        """awfmGpuChooseStrands: inputs strand_inputs(...) of the 2 num_reads rows (the reads as sequenced, then their reverse
        complements) and outputs strand_outputs(...) of device addresses; per read the strand and slot among its 2 max_candidates
        strand slots, best and second score and the mapping quality; paired (reads 2p and 2p + 1 are mates from opposite strands)
        also the pairing of pair_mates in both orientations and the rescue windows by row (what window_inputs takes on the
        2 num_reads rows); one launch, no scratch, asynchronous on `stream`; the counters are added to"""
        params = pair_params(min_insert, max_insert, min_score, unpaired_penalty, window_pad, mapq_cap)
        _check("awfmGpuChooseStrands",
               _lib.lib().awfmGpuChooseStrands(self.handle, C.byref(inputs), num_reads, max_candidates,
                                               (STRANDS_PAIRED if paired else 0) if flags is None else flags, C.byref(params),
                                               C.byref(outputs), stream or None))

    def orient_reads(self, inputs, num_reads, outputs, max_candidates=4, stream=0):
        """awfmGpuOrientReads: inputs orient_inputs(...) of the 2 num_reads rows and outputs orient_outputs(...) of device
        addresses; the chosen strand of every read -- characters, qualities (reversed on strand 1) and slot columns -- gathered
        into a batch of num_reads rows; one launch, asynchronous on `stream`; *numMalformed is added to"""
        _check("awfmGpuOrientReads",
               _lib.lib().awfmGpuOrientReads(self.handle, C.byref(inputs), num_reads, max_candidates, C.byref(outputs), stream or None))

    def locate_host_local(self, chars, offsets=None, fixed_length=0):
        """awfmGpuLocateHostLocal -> (ranges, hit offsets, sequence numbers uint32[total], local positions uint64[total],
        number of illegal positions)"""
        L = _lib.lib()
        chars = np.ascontiguousarray(chars, dtype=np.uint8)
        n = (len(offsets) - 1) if offsets is not None else chars.size // fixed_length
        ranges = np.zeros((n, 2), np.uint64)
        hit_off = np.zeros(n + 1, np.uint64)
        off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
        holder = chars if chars.size else np.zeros(1, np.uint8)
        seq_ptr, loc_ptr, illegal = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)(), C.c_uint64(0)
        rc = L.awfmGpuLocateHostLocal(self.handle, holder.ctypes.data, off.ctypes.data if off is not None else None, fixed_length, n,
                                      ranges.ctypes.data, hit_off.ctypes.data, C.byref(seq_ptr), C.byref(loc_ptr), C.byref(illegal))
        _check("awfmGpuLocateHostLocal", rc)
        total = int(hit_off[n])
        seq = np.ctypeslib.as_array(seq_ptr, shape=(total,)).copy() if total else np.zeros(0, np.uint32)
        loc = np.ctypeslib.as_array(loc_ptr, shape=(total,)).copy() if total else np.zeros(0, np.uint64)
        L.free(C.cast(seq_ptr, C.c_void_p))
        L.free(C.cast(loc_ptr, C.c_void_p))
        return ranges, hit_off, seq, loc, int(illegal.value)

    # host-buffer calls -------------------------------------------------
    def count_host(self, chars, offsets=None, fixed_length=0):
        chars = np.ascontiguousarray(chars, dtype=np.uint8)
        n = (len(offsets) - 1) if offsets is not None else chars.size // fixed_length
        ranges = np.zeros((n, 2), np.uint64)
        counts = np.zeros(n, np.uint32)
        off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
        holder = chars if chars.size else np.zeros(1, np.uint8)
        rc = _lib.lib().awfmGpuCountHost(self.handle, holder.ctypes.data, off.ctypes.data if off is not None else None,
                                         fixed_length, n, ranges.ctypes.data, counts.ctypes.data)
        _check("awfmGpuCountHost", rc)
        return ranges, counts

    def locate_host(self, chars, offsets=None, fixed_length=0):
        L = _lib.lib()
        chars = np.ascontiguousarray(chars, dtype=np.uint8)
        n = (len(offsets) - 1) if offsets is not None else chars.size // fixed_length
        ranges = np.zeros((n, 2), np.uint64)
        hit_off = np.zeros(n + 1, np.uint64)
        off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
        holder = chars if chars.size else np.zeros(1, np.uint8)
        pos_ptr = C.POINTER(C.c_uint64)()
        rc = L.awfmGpuLocateHost(self.handle, holder.ctypes.data, off.ctypes.data if off is not None else None,
                                 fixed_length, n, ranges.ctypes.data, hit_off.ctypes.data, C.byref(pos_ptr))
        _check("awfmGpuLocateHost", rc)
        total = int(hit_off[n])
        pos = np.ctypeslib.as_array(pos_ptr, shape=(total,)).copy() if total else np.zeros(0, np.uint64)
        L.free(C.cast(pos_ptr, C.c_void_p))
        return ranges, hit_off, pos

    def locate_host_windows(self, chars, offsets, sink):
        """awfmGpuLocateHostWindows: sink(user, query_begin, query_end, hit_begin, hit_end, positions) per window of the
        flat hit list; returns the hit offsets (uint64[n+1])"""
        chars = np.ascontiguousarray(chars, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(off) - 1
        hit_off = np.zeros(n + 1, np.uint64)
        holder = chars if chars.size else np.zeros(1, np.uint8)
        cb = _lib.HIT_WINDOW_SINK(sink)
        _check("awfmGpuLocateHostWindows", _lib.lib().awfmGpuLocateHostWindows(
            self.handle, holder.ctypes.data, off.ctypes.data, 0, n, None, hit_off.ctypes.data, cb, None))
        return hit_off

    # chunked pipeline on host buffers (awfm_gpu_stream.hip) ---------------------------
    def stream(self, kmers, kmer_length, locate=True, chunk=0, packed=True, threads=4, sink=None):
        """awfmGpuStreamPacked / awfmGpuStreamChars over a host array (numpy uint64[n] packed words, or uint8[n*L]
        ASCII; or an (address, n) pair for page-locked memory).  Without a sink the chunks are gathered:
        returns (counts uint32[n], positions uint64[total] or None)."""
        L = _lib.lib()
        if isinstance(kmers, tuple):
            address, n = kmers
        else:
            kmers = np.ascontiguousarray(kmers, dtype=np.uint64 if packed else np.uint8)
            n = kmers.size if packed else kmers.size // kmer_length
            address = kmers.ctypes.data if kmers.size else None
        counts = np.zeros(n, np.uint32)
        parts = []

        def gather(user, first, m, c, p, total):
            counts[first:first + m] = np.ctypeslib.as_array(c, shape=(m,))
            if locate and total:
                parts.append(np.ctypeslib.as_array(p, shape=(total,)).copy())
            return 0

        cb = _lib.CHUNK_SINK(sink or gather)
        fn = L.awfmGpuStreamPacked if packed else L.awfmGpuStreamChars
        _check(fn.__name__, fn(self.handle, address, kmer_length, n, chunk, int(bool(locate)), threads, cb, None))
        if sink is not None:
            return None
        return counts, (np.concatenate(parts) if parts else np.zeros(0, np.uint64)) if locate else None

    def stream_sparse(self, kmers, kmer_length, locate=True, chunk=0, packed=True, threads=4, sink=None):
        """awfmGpuStreamPackedSparse / awfmGpuStreamCharsSparse.  Without a sink the chunks are gathered: returns
        (hit_kmers uint64[m] batch-wide numbers, hit_offsets uint64[m+1], positions uint64[total] or None)."""
        L = _lib.lib()
        if isinstance(kmers, tuple):
            address, n = kmers
        else:
            kmers = np.ascontiguousarray(kmers, dtype=np.uint64 if packed else np.uint8)
            n = kmers.size if packed else kmers.size // kmer_length
            address = kmers.ctypes.data if kmers.size else None
        ids, lens, parts = [], [], []

        def gather(user, first, m, num, hit_kmers, hit_offsets, p, total):
            if num:
                ids.append(np.ctypeslib.as_array(hit_kmers, shape=(num,)).astype(np.uint64) + np.uint64(first))
                lens.append(np.diff(np.ctypeslib.as_array(hit_offsets, shape=(num + 1,))))
            if locate and total:
                parts.append(np.ctypeslib.as_array(p, shape=(total,)).copy())
            return 0

        cb = _lib.SPARSE_CHUNK_SINK(sink or gather)
        fn = L.awfmGpuStreamPackedSparse if packed else L.awfmGpuStreamCharsSparse
        _check(fn.__name__, fn(self.handle, address, kmer_length, n, chunk, int(bool(locate)), threads, cb, None))
        if sink is not None:
            return None
        hit_kmers = np.concatenate(ids) if ids else np.zeros(0, np.uint64)
        offsets = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.uint64) if lens else np.zeros(1, np.uint64)
        return hit_kmers, offsets, (np.concatenate(parts) if parts else np.zeros(0, np.uint64)) if locate else None

    def count_packed_host(self, packed, kmer_length):
        packed = np.ascontiguousarray(packed, dtype=np.uint64)
        counts = np.zeros(packed.size, np.uint32)
        _check("awfmGpuCountPackedHost", _lib.lib().awfmGpuCountPackedHost(
            self.handle, packed.ctypes.data if packed.size else None, kmer_length, packed.size, counts.ctypes.data))
        return counts

    def locate_packed_host(self, packed, kmer_length):
        L = _lib.lib()
        packed = np.ascontiguousarray(packed, dtype=np.uint64)
        counts = np.zeros(packed.size, np.uint32)
        pos_ptr, total = C.POINTER(C.c_uint64)(), C.c_uint64(0)
        _check("awfmGpuLocatePackedHost", L.awfmGpuLocatePackedHost(
            self.handle, packed.ctypes.data if packed.size else None, kmer_length, packed.size, counts.ctypes.data,
            C.byref(pos_ptr), C.byref(total)))
        pos = np.ctypeslib.as_array(pos_ptr, shape=(total.value,)).copy() if total.value else np.zeros(0, np.uint64)
        L.free(C.cast(pos_ptr, C.c_void_p))
        return counts, pos

    def pack_device(self, d_chars, kmer_length, n, d_packed, stream=0):
        """awfmGpuPackKmers on device buffers; returns how many k-mers could not be expressed (the library call itself
        reports AwFmIllegalPositionError then: the packed words of such a batch must not be searched)"""
        bad = C.c_uint64(0)
        rc = _lib.lib().awfmGpuPackKmers(self.handle, d_chars, kmer_length, n, d_packed, C.byref(bad), stream or None)
        if rc == AwFmIllegalPositionError and bad.value:
            return int(bad.value)
        _check("awfmGpuPackKmers", rc)
        return int(bad.value)

    def unpack_device(self, d_packed, kmer_length, n, d_chars, stream=0):
        _check("awfmGpuUnpackKmers", _lib.lib().awfmGpuUnpackKmers(self.handle, d_packed, kmer_length, n, d_chars, stream or None))

    # device-pointer calls (addresses as ints, e.g. torch tensor.data_ptr()) -------------
    def search(self, d_chars, d_offsets, fixed_length, n, d_ranges, d_counts, stream=0):
        _check("awfmGpuSearch", _lib.lib().awfmGpuSearch(self.handle, d_chars, d_offsets or None, fixed_length, n,
                                                         d_ranges or None, d_counts or None, stream or None))

    def longest_suffix_matches(self, d_chars, d_starts, d_ends, fixed_length, n, min_length, d_lengths, d_ranges, d_counts, stream=0):
        """awfmGpuLongestSuffixMatches: per query chars[starts[i]:ends[i]] (d_starts = d_ends = 0: fixed_length characters each)
        the length of its longest suffix that occurs, that suffix's range and count; each output may be 0"""
        _check("awfmGpuLongestSuffixMatches", _lib.lib().awfmGpuLongestSuffixMatches(
            self.handle, d_chars, d_starts or None, d_ends or None, fixed_length, n, min_length, d_lengths or None, d_ranges or None,
            d_counts or None, stream or None))

    def one_substitution_search(self, d_chars, d_offsets, fixed_length, n, include_exact, d_hit_queries, d_hit_edits, d_hit_ranges,
                                capacity, d_num_hits, d_variants, d_occurrences, stream=0):
        """awfmGpuOneSubstitutionSearch on device addresses (0: NULL): the records {query, edit, range} of every string at
        Hamming distance 1 of query i = chars[offsets[i]:offsets[i + 1]] (d_offsets = 0: fixed_length characters each) appended
        to lists of `capacity` entries that were first filled with "no record"; *d_num_hits (uint64) = the true number of
        records, d_variants (uint32[n]) / d_occurrences (uint64[n]) = records and summed range lengths per query.
        Asynchronous on `stream`."""
        _check("awfmGpuOneSubstitutionSearch", _lib.lib().awfmGpuOneSubstitutionSearch(
            self.handle, d_chars, d_offsets, fixed_length, n, 1 if include_exact else 0, d_hit_queries, d_hit_edits, d_hit_ranges,
            capacity, d_num_hits, d_variants, d_occurrences, stream))

    def search_hits(self, d_chars, d_offsets, fixed_length, n, d_ranges, d_counts, stream=0):
        """awfmGpuSearchHits: like search(), but a query without hits only gets count 0 and some empty range"""
        _check("awfmGpuSearchHits", _lib.lib().awfmGpuSearchHits(self.handle, d_chars, d_offsets or None, fixed_length,
                                                                 n, d_ranges or None, d_counts or None, stream or None))

    def search_hits_sparse(self, d_chars, d_offsets, fixed_length, n, d_ranges, d_counts, stream=0):
        """awfmGpuSearchHitsSparse: counts for every query, ranges only for the queries with hits (the others' may stay
        as passed); hit offsets then come from the counts"""
        _check("awfmGpuSearchHitsSparse", _lib.lib().awfmGpuSearchHitsSparse(self.handle, d_chars, d_offsets or None, fixed_length,
                                                                            n, d_ranges or None, d_counts, stream or None))

    def search_hits_packed(self, d_packed, kmer_length, n, d_ranges, d_counts, d_chars_scratch=0, stream=0):
        """awfmGpuSearchHitsPacked: hits-only search of bit-packed k-mers resident on the device"""
        _check("awfmGpuSearchHitsPacked", _lib.lib().awfmGpuSearchHitsPacked(
            self.handle, d_packed, kmer_length, n, d_ranges or None, d_counts or None, d_chars_scratch or None, stream or None))

    def search_hits_compact(self, d_chars, d_offsets, fixed_length, n, d_hit_kmers, d_hit_ranges, capacity, d_num_hits,
                            packed=False, stream=0):
        """awfmGpuSearchHitsCompact: the k-mers with hits appended to a list (seed-order path only)"""
        _check("awfmGpuSearchHitsCompact", _lib.lib().awfmGpuSearchHitsCompact(
            self.handle, d_chars, d_offsets or None, fixed_length, n, int(bool(packed)), d_hit_kmers, d_hit_ranges, capacity,
            d_num_hits, stream or None))

    # seed-bucket sharding (include/awfm_gpu.h) ---------------------------
    def order_buckets(self, fixed_length, total_queries):
        """buckets of the seed order of such a batch on this image (0: not a batch for 8-byte records)"""
        return int(_lib.lib().awfmGpuOrderBuckets(self.handle, fixed_length, total_queries))

    def order_kmers(self, d_chars, fixed_length, n, first_number, total_queries, d_records, d_bucket_start, stream=0):
        """awfmGpuOrderKmers: the shard's records {rest of the code string, number in the whole batch} in bucket order"""
        _check("awfmGpuOrderKmers", _lib.lib().awfmGpuOrderKmers(self.handle, d_chars, fixed_length, n, first_number, total_queries,
                                                               d_records, d_bucket_start, stream or None))

    def search_ordered_records(self, d_records, d_bucket_start, first_bucket, end_bucket, fixed_length, total_queries, d_order_kmers,
                               d_order_ranges, stream=0, d_order_counts=0):
        """awfmGpuSearchOrderedRecords[Counts]: the buckets [first, end) of a record array, results in that order (d_order_counts:
        the 32-bit counts in that order as well)"""
        _check("awfmGpuSearchOrderedRecordsCounts", _lib.lib().awfmGpuSearchOrderedRecordsCounts(
            self.handle, d_records, d_bucket_start, first_bucket, end_bucket, fixed_length, total_queries, d_order_kmers, d_order_ranges,
            d_order_counts or None, stream or None))

    def merge_bucket_runs(self, d_received, d_slice_at, d_slice_starts, num_slices, first_bucket, end_bucket, buckets, d_records,
                          d_bucket_start, stream=0):
        """awfmGpuMergeBucketRuns: the slices a rank received in the exchange of the seed-bucket sharding, put in bucket order
        (one launch), with the bucket starts search_ordered_records wants"""
        _check("awfmGpuMergeBucketRuns", _lib.lib().awfmGpuMergeBucketRuns(
            self.handle, d_received, d_slice_at, d_slice_starts, num_slices, first_bucket, end_bucket, buckets, d_records, d_bucket_start,
            stream or None))

    def search_general_records(self, d_chars, fixed_length, n, first_number, total_queries, d_records, d_bucket_start, d_order_kmers,
                               d_order_ranges, stream=0):
        """awfmGpuSearchGeneralRecords: the tail of a shard's own records (k-mers with ambiguity characters) through the general kernel"""
        _check("awfmGpuSearchGeneralRecords", _lib.lib().awfmGpuSearchGeneralRecords(
            self.handle, d_chars, fixed_length, n, first_number, total_queries, d_records, d_bucket_start, d_order_kmers, d_order_ranges,
            stream or None))

    def search_hits_in_order(self, d_chars, d_offsets, fixed_length, n, d_order_kmers, d_order_ranges, packed=False, stream=0,
                             d_order_counts=0):
        """awfmGpuSearchHitsInOrder[Counts]: {k-mer number, range} for every k-mer, in the order the seed-order search took them;
        d_order_counts: the 32-bit counts in that order as well"""
        _check("awfmGpuSearchHitsInOrderCounts", _lib.lib().awfmGpuSearchHitsInOrderCounts(
            self.handle, d_chars, d_offsets or None, fixed_length, n, int(bool(packed)), d_order_kmers, d_order_ranges,
            d_order_counts or None, stream or None))

    def compact_hits(self, d_counts, d_ranges, n, d_flag_offsets, d_scratch, d_hit_kmers, d_hit_ranges, capacity, d_num_hits,
                     stream=0):
        _check("awfmGpuCompactHits", _lib.lib().awfmGpuCompactHits(self.handle, d_counts, d_ranges, n, d_flag_offsets, d_scratch,
                                                                   d_hit_kmers, d_hit_ranges, capacity, d_num_hits, stream or None))

    def sort_hits(self, d_hit_kmers, d_hit_ranges, num_entries, stream=0):
        _check("awfmGpuSortHits", _lib.lib().awfmGpuSortHits(self.handle, d_hit_kmers, d_hit_ranges, num_entries, stream or None))

    def sort_hits_on_device(self, d_hit_kmers, d_hit_ranges, capacity, d_num_hits, n, stream=0):
        """awfmGpuSortHitsOnDevice: the list in k-mer order, its length read on the device (no host wait)"""
        _check("awfmGpuSortHitsOnDevice", _lib.lib().awfmGpuSortHitsOnDevice(self.handle, d_hit_kmers, d_hit_ranges, capacity,
                                                                             d_num_hits, n, stream or None))

    def describe(self):
        """awfmGpuIndexDescribe: one line about what the image holds and which accelerators it did not get"""
        import ctypes as C
        buf = C.create_string_buffer(2048)
        _lib.lib().awfmGpuIndexDescribe(self.handle, buf, 2048)
        return buf.value.decode()

    def stream_retire(self, stream):
        """awfmGpuStreamRetire: call before destroying a stream that has searched on this image"""
        _lib.lib().awfmGpuStreamRetire(self.handle, stream or None)

    def last_lookup_front(self):
        """awfmGpuLastLookupFront: 0 both front ends, 1 the lookup kernel only, 2 the ordered kernels only, -1 none yet"""
        return int(_lib.lib().awfmGpuLastLookupFront(self.handle))

    def last_search_was_exact_lookup(self):
        """awfmGpuLastSearchWasExactLookup: the last awfmGpuSearch took exactLookupSearchKernel"""
        return bool(_lib.lib().awfmGpuLastSearchWasExactLookup(self.handle))

    def list_locate_on_device(self, d_hit_kmers, d_hit_ranges, capacity, d_num_hits, n, d_sorted_kmers, d_sorted_ranges, d_hit_offsets,
                              capacity_hits, d_positions, stream=0):
        """awfmGpuListLocateOnDevice: the appended list -> the list in k-mer order, its hit offsets and positions, in one launch"""
        _check("awfmGpuListLocateOnDevice", _lib.lib().awfmGpuListLocateOnDevice(
            self.handle, d_hit_kmers, d_hit_ranges, capacity, d_num_hits, n, d_sorted_kmers, d_sorted_ranges, d_hit_offsets,
            capacity_hits, d_positions or None, stream or None))

    def hit_offsets_on_device(self, d_counts, d_ranges, n, d_hit_offsets, d_scratch, stream=0):
        """awfmGpuHitOffsetsOnDevice: the scan; the total stays in d_hit_offsets[n]"""
        _check("awfmGpuHitOffsetsOnDevice", _lib.lib().awfmGpuHitOffsetsOnDevice(self.handle, d_counts or None, d_ranges or None, n,
                                                                                 d_hit_offsets, d_scratch, stream or None))

    def locate_on_device(self, d_ranges, d_hit_offsets, n, capacity_hits, d_positions, stream=0):
        """awfmGpuLocateOnDevice: the locate with the number of hits read on the device, at most capacity_hits of them"""
        _check("awfmGpuLocateOnDevice", _lib.lib().awfmGpuLocateOnDevice(self.handle, d_ranges, d_hit_offsets, n, capacity_hits,
                                                                         d_positions, stream or None))

    def ordered_kernel_log(self, max_entries=1024):
        """awfmGpuOrderedKernelLog: [(encodeLookupKernel ms or -1, orderedSearchKernel ms or -1)] of the searches timed since
        the last call ($AWFM_GPU_TIME_ORDERED), oldest first"""
        front = (C.c_double * max_entries)()
        kern = (C.c_double * max_entries)()
        n = _lib.lib().awfmGpuOrderedKernelLog(self.handle, front, kern, max_entries)
        return [(front[i], kern[i]) for i in range(n)]

    def last_ordered_search_kernel_ms(self):
        return float(_lib.lib().awfmGpuLastOrderedSearchKernelMs(self.handle))

    def search_hits_is_ordered(self, has_offsets, fixed_length, n):
        return bool(_lib.lib().awfmGpuSearchHitsIsOrdered(self.handle, int(bool(has_offsets)), fixed_length, n))

    def last_ordered_kernel_ms(self):
        return float(_lib.lib().awfmGpuLastOrderedKernelMs(self.handle))

    def last_ordered_kept(self):
        """k-mers the last seed-order search with 8-byte records ordered and searched (awfmGpuLastOrderedKept)"""
        return int(_lib.lib().awfmGpuLastOrderedKept(self.handle))

    def last_second_window(self):
        """(tested, dropped): the survivors the lookup kernel of the last seed-order search put to its second table window, and
        those it dropped there (awfmGpuLastSecondWindow)"""
        out = (C.c_uint64 * 2)()
        _lib.lib().awfmGpuLastSecondWindow(self.handle, C.byref(out))
        return int(out[0]), int(out[1])

    def last_ordered_kernel_is_lookup(self):
        """the kernel last_ordered_kernel_ms() timed was encodeLookupKernel ("lookup first", include/awfm_gpu.h)"""
        return bool(_lib.lib().awfmGpuLastOrderedKernelIsLookup(self.handle))

    def set_ordered(self, mode):
        """-1 automatic, 0 never, 1 always: search_hits() of fixed-length nucleotide batches in seed order"""
        _lib.lib().awfmGpuIndexSetOrdered(self.handle, mode)

    def search_tally(self, d_chars, d_offsets, fixed_length, n):
        """{seeded, steps, blocks, chars} of the instrumented search kernel"""
        out = (C.c_uint64 * 4)()
        _check("awfmGpuSearchTally", _lib.lib().awfmGpuSearchTally(self.handle, d_chars, d_offsets or None, fixed_length,
                                                                   n, C.byref(out)))
        return {"seeded": int(out[0]), "steps": int(out[1]), "blocks": int(out[2]), "chars": int(out[3])}

    def search_hits_line_tally(self, d_chars, d_offsets, fixed_length, n):
        """compulsory traffic of the seed-order search of this batch (awfmGpuSearchHitsLineTally): distinct 128-B lines
        per search level, records read, results stored"""
        out = (C.c_uint64 * 8)()
        _check("awfmGpuSearchHitsLineTally", _lib.lib().awfmGpuSearchHitsLineTally(self.handle, d_chars, d_offsets or None,
                                                                                   fixed_length, n, C.byref(out)))
        keys = ("seed_table_lines", "deep_table_lines", "pair_level_lines", "nuc_level_lines", "ordered_kmers",
                "record_bytes_per_kmer", "kmers_with_hits", "general_kmers")
        return {k: int(v) for k, v in zip(keys, out)}

    def hit_offsets(self, d_ranges, n, d_hit_offsets, d_scratch, stream=0):
        total = C.c_uint64(0)
        _check("awfmGpuHitOffsets", _lib.lib().awfmGpuHitOffsets(self.handle, d_ranges, n, d_hit_offsets, d_scratch,
                                                                 C.byref(total), stream or None))
        return int(total.value)

    def hit_offsets_from_counts(self, d_counts, n, d_hit_offsets, d_scratch, stream=0):
        total = C.c_uint64(0)
        _check("awfmGpuHitOffsetsFromCounts", _lib.lib().awfmGpuHitOffsetsFromCounts(
            self.handle, d_counts, n, d_hit_offsets, d_scratch, C.byref(total), stream or None))
        return int(total.value)

    def locate(self, d_ranges, d_hit_offsets, n, total_hits, d_positions, stream=0):
        _check("awfmGpuLocate", _lib.lib().awfmGpuLocate(self.handle, d_ranges, d_hit_offsets, n, total_hits,
                                                         d_positions, stream or None))

    def locate_window(self, d_ranges, d_hit_offsets, query_begin, query_end, hit_begin, hit_end, d_positions, stream=0):
        """awfmGpuLocateWindow: the hits numbered hit_begin .. hit_end-1 of the batch's flat hit list"""
        _check("awfmGpuLocateWindow", _lib.lib().awfmGpuLocateWindow(self.handle, d_ranges, d_hit_offsets, query_begin, query_end,
                                                                     hit_begin, hit_end, d_positions, d_positions, stream or None))

    @staticmethod
    def scan_scratch_bytes(n):
        return int(_lib.lib().awfmGpuScanScratchBytes(n))

    def destroy(self):
        if self.handle:
            if self.owned:
                _lib.lib().awfmGpuIndexDestroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
