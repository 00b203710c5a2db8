"""ctypes binding of the reference itself, compiled by oracle/Makefile into oracle/_ref/libawfm_ref.so.

TEST INFRASTRUCTURE ONLY.  The library exists only where the reference's sources are mounted (the CPU machine); it is
neither committed nor carried to a GPU machine -- there its answers arrive as the fixtures tests/golden/ref_*.npz that
scripts/make_reference_golden.py records through this module.

Index is shaped like oracle.oracle.Index so that a test can put the two side by side.  The structs are those of
avxwindowfmindex_amd/_lib.py: the ABI of the product is the reference's (tests/test_host_lib.py pins it).
"""
import ctypes as C
import os
import tempfile

import numpy as np

from avxwindowfmindex_amd import _lib as P

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libawfm_ref.so")
SOURCE_DIR = os.path.join(os.environ.get("REF", "/root/reference"), "src")  # oracle/Makefile's REF, same default and override
_LIB = None

AMINO, DNA = 1, 2
CONCURRENT_QUERIES = 32  # the reference's block of k-mers per thread (AW_FM_NUM_CONCURRENT_QUERIES)

# struct AwFmKmerSearchData as a numpy record, to fill and read a whole list at once
KMER_DTYPE = np.dtype([("kmerString", np.uint64), ("kmerLength", np.uint64), ("positionList", np.uint64),
                       ("count", np.uint32), ("capacity", np.uint32)])
assert KMER_DTYPE.itemsize == C.sizeof(P.AwFmKmerSearchData)


def available():
    return os.path.exists(LIB_PATH)


def sources_present():
    return os.path.isdir(SOURCE_DIR)


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not available():
        raise RuntimeError("oracle/_ref/libawfm_ref.so is not built (make -C oracle _ref/libawfm_ref.so, where the "
                           "reference's sources are present)")
    L = C.CDLL(LIB_PATH)  # RTLD_LOCAL: its awFm* names must not shadow the product's
    IP, LP, RP = C.POINTER(P.AwFmIndex), C.POINTER(P.AwFmKmerSearchList), C.POINTER(P.AwFmSearchRange)
    u64 = C.c_uint64
    sig = {
        "awFmCreateIndex": (C.c_int, [C.POINTER(IP), C.POINTER(P.AwFmIndexConfiguration), C.c_void_p, C.c_size_t, C.c_char_p]),
        "awFmDeallocIndex": (None, [IP]),
        "awFmReadIndexFromFile": (C.c_int, [C.POINTER(IP), C.c_char_p, C.c_bool]),
        "awFmCreateKmerSearchList": (LP, [C.c_size_t]),
        "awFmDeallocKmerSearchList": (None, [LP]),
        "awFmParallelSearchLocate": (C.c_int, [IP, LP, C.c_uint32]),
        "awFmParallelSearchCount": (None, [IP, LP, C.c_uint32]),
        "parallelSearchFindKmerSeedsForBlock": (None, [IP, LP, RP, C.c_size_t, C.c_size_t]),
        "parallelSearchExtendKmersInBlock": (None, [IP, LP, RP, C.c_size_t, C.c_size_t]),
        "awFmFindSearchRangeForString": (P.AwFmSearchRange, [IP, C.c_char_p, C.c_size_t]),
        "awFmReadSequenceFromFile": (C.c_int, [IP, C.c_size_t, C.c_size_t, C.c_char_p]),
        "awFmCreateInitialQueryRange": (P.AwFmSearchRange, [IP, C.c_char_p, u64]),
        "awFmCreateInitialQueryRangeFromChar": (P.AwFmSearchRange, [IP, C.c_char]),
        "awFmNucleotideIterativeStepBackwardSearch": (None, [IP, RP, C.c_uint8]),
        "awFmAminoIterativeStepBackwardSearch": (None, [IP, RP, C.c_uint8]),
        "awFmFindDatabaseHitPositionSingle": (u64, [IP, u64, C.POINTER(C.c_int)]),
        "awFmNucleotideBacktraceReturnPreviousLetterIndex": (C.c_uint8, [IP, C.POINTER(u64)]),
        "awFmAminoBacktraceReturnPreviousLetterIndex": (C.c_uint8, [IP, C.POINTER(u64)]),
        "awFmAsciiNucleotideToLetterIndex": (C.c_uint8, [C.c_uint8]),
        "awFmAsciiAminoAcidToLetterIndex": (C.c_uint8, [C.c_uint8]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _LIB = L
    return L


class SearchList:
    """struct AwFmKmerSearchList* of the reference's own allocator, filled from (chars, offsets) in one go"""

    def __init__(self, chars, offsets):
        self.chars = np.ascontiguousarray(chars, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.n = len(offsets) - 1
        self.ptr = lib().awFmCreateKmerSearchList(max(self.n, 1))
        if not self.ptr:
            raise MemoryError("awFmCreateKmerSearchList")
        self.ptr.contents.count = self.n
        rec = self.records()
        rec["kmerString"] = np.uint64(self.chars.ctypes.data) + offsets[:-1]
        rec["kmerLength"] = np.diff(offsets)

    def records(self):
        """the kmerSearchData array as a numpy record view (live memory)"""
        address = C.cast(self.ptr.contents.kmerSearchData, C.c_void_p).value
        buf = (C.c_uint8 * (self.n * KMER_DTYPE.itemsize)).from_address(address)
        return np.frombuffer(buf, dtype=KMER_DTYPE, count=self.n)

    def counts(self):
        return self.records()["count"].copy()

    def positions(self):
        """(hit offsets uint64[n+1], positions uint64[total]) in list order"""
        rec = self.records()
        counts = rec["count"].astype(np.uint64)
        hit_off = np.zeros(self.n + 1, np.uint64)
        np.cumsum(counts, out=hit_off[1:])
        parts = [np.frombuffer(C.string_at(int(p), int(c) * 8), np.uint64) for p, c in zip(rec["positionList"], counts) if c]
        return hit_off, (np.concatenate(parts) if parts else np.zeros(0, np.uint64))

    def free(self):
        if self.ptr:
            lib().awFmDeallocKmerSearchList(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Index:
    """struct AwFmIndex* made by the reference's awFmCreateIndex or awFmReadIndexFromFile"""

    def __init__(self, ptr, file_src, owns_file=False):
        self.ptr = ptr
        self.file_src = file_src
        self._owns_file = owns_file

    @classmethod
    def from_text(cls, text, alphabet, sa_ratio, seed_k, file_src=None, keep_sa_in_memory=True, store_sequence=False):
        t = np.frombuffer(bytes(text), dtype=np.uint8).copy()
        if t.size == 0:
            raise ValueError("the reference evaluates clz(0) on an empty text")
        owns = file_src is None
        if owns:
            fd, file_src = tempfile.mkstemp(suffix=".awfmi", prefix="awfm_ref_")
            os.close(fd)
        cfg = P.AwFmIndexConfiguration(sa_ratio, seed_k, alphabet, keep_sa_in_memory, store_sequence)
        out = C.POINTER(P.AwFmIndex)()
        rc = lib().awFmCreateIndex(C.byref(out), C.byref(cfg), t.ctypes.data, t.size, file_src.encode())
        if rc != P.AwFmFileWriteOkay:
            raise RuntimeError(f"reference awFmCreateIndex returned {rc}")
        return cls(out, file_src, owns)

    @classmethod
    def from_file(cls, file_src, keep_sa_in_memory=True):
        out = C.POINTER(P.AwFmIndex)()
        rc = lib().awFmReadIndexFromFile(C.byref(out), file_src.encode(), keep_sa_in_memory)
        if rc != P.AwFmFileReadOkay:
            raise RuntimeError(f"reference awFmReadIndexFromFile returned {rc}")
        return cls(out, file_src)

    def free(self):
        if self.ptr:
            lib().awFmDeallocIndex(self.ptr)
            self.ptr = None
            if self._owns_file and os.path.exists(self.file_src):
                os.unlink(self.file_src)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    # --- arrays, reference layout (copies) ---
    @property
    def c(self):
        return self.ptr.contents

    @property
    def bwt_length(self):
        return int(self.c.bwtLength)

    @property
    def is_amino(self):
        return self.c.config.alphabetType == AMINO

    @property
    def sa_ratio(self):
        return int(self.c.config.suffixArrayCompressionRatio)

    @property
    def sa_width(self):
        return int(self.c.suffixArray.valueBitWidth)

    def blocks(self):
        nbytes = (1 + (self.bwt_length - 1) // 256) * (352 if self.is_amino else 160)
        return np.ctypeslib.as_array(C.cast(self.c.bwtBlockList, C.POINTER(C.c_uint8)), shape=(nbytes,)).copy()

    def prefix_sums(self):
        return np.ctypeslib.as_array(self.c.prefixSums, shape=((20 if self.is_amino else 4) + 2,)).copy()

    def seed_table(self):
        n = (20 if self.is_amino else 4) ** int(self.c.config.kmerLengthInSeedTable)
        return np.ctypeslib.as_array(C.cast(self.c.kmerSeedTable, C.POINTER(C.c_uint64)), shape=(n, 2)).copy()

    def packed_sa(self):
        """all compressedByteLength bytes, the 8 padding bytes at the end included"""
        sa = self.c.suffixArray
        if not sa.values:
            return None
        return np.ctypeslib.as_array(sa.values, shape=(int(sa.compressedByteLength),)).copy()

    # --- single-query functions ---
    def letter_index(self, ascii_code):
        f = lib().awFmAsciiAminoAcidToLetterIndex if self.is_amino else lib().awFmAsciiNucleotideToLetterIndex
        return int(f(ascii_code))

    def range_for_string(self, kmer):
        r = lib().awFmFindSearchRangeForString(self.ptr, bytes(kmer), len(kmer))
        return int(r.startPtr), int(r.endPtr)

    def initial_range(self, query):
        """awFmCreateInitialQueryRange: the range of the query's last letter"""
        r = lib().awFmCreateInitialQueryRange(self.ptr, bytes(query), len(query))
        return int(r.startPtr), int(r.endPtr)

    def initial_range_from_char(self, letter):
        r = lib().awFmCreateInitialQueryRangeFromChar(self.ptr, bytes(letter[:1]))
        return int(r.startPtr), int(r.endPtr)

    def step(self, sp, ep, letter_index):
        r = P.AwFmSearchRange(sp, ep)
        f = lib().awFmAminoIterativeStepBackwardSearch if self.is_amino else lib().awFmNucleotideIterativeStepBackwardSearch
        f(self.ptr, C.byref(r), letter_index)
        return int(r.startPtr), int(r.endPtr)

    def locate_one(self, bwt_position):
        rc = C.c_int(0)
        return int(lib().awFmFindDatabaseHitPositionSingle(self.ptr, bwt_position, C.byref(rc)))

    def locate_all(self):
        """text position of every BWT position 0 .. bwtLength-1"""
        f, rc, ptr = lib().awFmFindDatabaseHitPositionSingle, C.c_int(0), self.ptr
        return np.array([f(ptr, p, C.byref(rc)) for p in range(self.bwt_length)], dtype=np.uint64)

    def previous_letter(self, bwt_position):
        """-> (letter index, BWT position of the previous letter)"""
        p = C.c_uint64(bwt_position)
        f = (lib().awFmAminoBacktraceReturnPreviousLetterIndex if self.is_amino
             else lib().awFmNucleotideBacktraceReturnPreviousLetterIndex)
        letter = f(self.ptr, C.byref(p))
        return int(letter), int(p.value)

    def read_sequence(self, start, length):
        """awFmReadSequenceFromFile -> (return code, bytes)"""
        buf = C.create_string_buffer(length + 1)
        rc = lib().awFmReadSequenceFromFile(self.ptr, start, length, buf)
        return rc, buf.raw[:length]

    # --- batches ---
    def batch_search(self, chars, offsets, threads=1):
        """exact {sp, ep} of every query -- the absent ones too -- from the two functions awFmParallelSearchCount runs
        per block of 32 k-mers, and the counts of awFmParallelSearchCount itself -> (sp, ep, counts, None)"""
        L = lib()
        sl = SearchList(chars, offsets)
        n = sl.n
        ranges = np.zeros((n + CONCURRENT_QUERIES, 2), np.uint64)
        for first in range(0, n, CONCURRENT_QUERIES):
            end = min(first + CONCURRENT_QUERIES, n)
            block = C.cast(ranges[first:].ctypes.data, C.POINTER(P.AwFmSearchRange))
            L.parallelSearchFindKmerSeedsForBlock(self.ptr, sl.ptr, block, first, end)
            L.parallelSearchExtendKmersInBlock(self.ptr, sl.ptr, block, first, end)
        L.awFmParallelSearchCount(self.ptr, sl.ptr, threads)
        counts = sl.counts()
        sl.free()
        return ranges[:n, 0].copy(), ranges[:n, 1].copy(), counts, None

    def batch_locate(self, chars, offsets, threads=1):
        """awFmParallelSearchLocate -> (hit offsets uint64[n+1], positions in list order, return code)"""
        sl = SearchList(chars, offsets)
        rc = lib().awFmParallelSearchLocate(self.ptr, sl.ptr, threads)
        hit_off, pos = sl.positions()
        sl.free()
        return hit_off, pos, rc

    def search_list(self, queries, threads=1):
        from oracle.oracle import pack_queries
        chars, offsets = pack_queries(queries)
        return self.batch_search(chars, offsets, threads)
