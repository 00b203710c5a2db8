#!/usr/bin/env python3
"""Records tests/golden/ref_*.npz: what the reference itself (oracle/_ref/libawfm_ref.so, see oracle/Makefile) answers on
the small cases of tests/reference_common.FIXTURE_CASES, for the machines the reference does not travel to.

Each file holds the text, the queries, the bytes of the .awfmi file the reference wrote, the digests of its four arrays,
the exact range of every query, counts, hit offsets and positions in list order, the (length, range) of the walk over its
step functions per query, and the text position of every BWT position.  tests/test_reference_parity.py regenerates every
file's content from the live reference and compares, so the fixtures cannot drift.  The fixtures are data; this script
is their provenance.  Usage, where the reference library is built: python scripts/make_reference_golden.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import longest_match_common as lm  # noqa: E402
import reference_common as rc  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import reference as R  # noqa: E402


def record(case):
    """-> dict of arrays, the content of the case's .npz"""
    name, alpha, kind, n, ratio, seed_k, nq = case
    text, queries = rc.fixture_inputs(case)
    chars, offsets = rc.pack(queries)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, name + ".awfmi")
        ri = R.Index.from_text(text, R.AMINO if alpha == "amino" else R.DNA, ratio, seed_k, file_src=path)
        blob = np.fromfile(path, dtype=np.uint8)
    sp, ep, counts, _ = ri.batch_search(chars, offsets)
    hit_off, positions, code = ri.batch_locate(chars, offsets)
    assert code == 1
    walk = [lm.step_walk(R.lib(), ri, q) for q in queries]
    out = dict(
        text=np.frombuffer(text, np.uint8), chars=chars, offsets=offsets, awfmi=blob,
        config=np.array([R.AMINO if alpha == "amino" else R.DNA, ratio, seed_k, ri.bwt_length, ri.sa_width], np.uint64),
        digests=np.array([O.fnv1a(ri.blocks()), O.fnv1a(ri.prefix_sums()), O.fnv1a(ri.seed_table())], np.uint64),
        samples=rc.sa_samples(ri.packed_sa(), ri.bwt_length, ratio),
        sp=sp, ep=ep, count=counts, hit_offsets=hit_off, positions=positions,
        walk_length=np.array([w[0] for w in walk], np.uint32), walk_range=np.array([w[1] for w in walk], np.uint64),
        all_positions=ri.locate_all())
    ri.free()
    return out


def main():
    total = 0
    for case in rc.FIXTURE_CASES:
        path = os.path.join(rc.GOLDEN_DIR, case[0] + ".npz")
        data = record(case)
        np.savez_compressed(path, **data)
        total += os.path.getsize(path)
        print(case[0], "queries", len(data["sp"]), "hits", len(data["positions"]), "awfmi", len(data["awfmi"]), "bytes",
              os.path.getsize(path))
    print("total", total)


if __name__ == "__main__":
    main()
