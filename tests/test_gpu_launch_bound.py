"""GPU: found-list calls whose work exceeds one kernel launch.  HIP takes at most 2^32 - 1 work-items per grid dimension; 96 000 sequences of one length make about
72 M tiles of 64 candidates, above the 67.1 M tiles (four per 256-thread workgroup) that fit one launch - the smallest shape at which the bound matters.  The set:
24 letters each, the first 8 shared (one seed bucket for umi_pairs at seed_len 8), random behind, 500 planted exact duplicates with partners over the whole index
range.  Expected: the identical-sequence pairs by np.unique on the host; every comparison exact."""
import functools
import numpy as np
import pytest
import variants_reference as ref
from ngspeciesid_amd._capi import ReadSet

pytestmark = pytest.mark.gpu
N, LEN, SHARED, PLANTED = 96_000, 24, 8, 500


@functools.lru_cache(maxsize=None)
def _set():
    """-> (letters uint8 [N, LEN], planted pairs [(i, j)], every pair i < j of identical rows in ascending (i, j) order as int64 [P, 2])"""
    rng = np.random.default_rng(96)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(N, LEN))]
    letters[:, :SHARED] = letters[0, :SHARED]
    # copies: 60 among the last 1 000 indices, the others anywhere behind the first 1 000; originals: an index below the copy's own, over the whole range
    dst = np.concatenate([rng.choice(np.arange(N - 1000, N), 60, replace=False), rng.choice(np.arange(1000, N - 1000), PLANTED - 60, replace=False)])
    src = np.array([int(rng.integers(0, j)) for j in dst.tolist()])
    keep = ~np.isin(src, dst)                                      # an original that is itself a copy would make the planted list depend on the order of copying
    src[~keep] = np.arange(int((~keep).sum()))                     # (indices below 1 000: never a copy)
    letters[dst] = letters[src]
    planted = sorted(zip(src.tolist(), dst.tolist()))
    assert len(planted) == PLANTED and sum(j >= N - 1000 for _, j in planted) >= 50 and all(i < j for i, j in planted)
    _, inv, cnt = np.unique(np.ascontiguousarray(letters).view("V%d" % LEN).ravel(), return_inverse=True, return_counts=True)
    inv = inv.ravel()
    rows = np.flatnonzero(cnt[inv] > 1)                            # ascending indices of the rows that have a twin
    groups = {}
    for r in rows.tolist(): groups.setdefault(int(inv[r]), []).append(r)
    pairs = sorted((g[a], g[b]) for g in groups.values() for a in range(len(g)) for b in range(a + 1, len(g)))
    assert set(planted) <= set(pairs)
    letters.setflags(write=False)
    return letters, planted, np.array(pairs, dtype=np.int64)


def _reads():
    letters = _set()[0]
    return ReadSet(letters.ravel(), None, np.arange(N + 1, dtype=np.uint64) * LEN)


def _assert_exact(got_i, got_j, got_dist, want, what):
    print("%s: %d pairs, want %d" % (what, len(got_i), len(want)))
    assert got_i.dtype == np.uint32 and got_j.dtype == np.uint32 and got_dist.dtype == np.uint8
    assert len(got_i) == len(want), "%s: %d pairs, want %d" % (what, len(got_i), len(want))
    assert np.array_equal(got_i, want[:, 0]) and np.array_equal(got_j, want[:, 1]) and not got_dist.any(), what


def test_near_pairs_beyond_one_launch(gpu_api):
    want = _set()[2]
    pi, pj, dist, strand = gpu_api.near_pairs(_reads(), 0, both_strands=False)
    _assert_exact(pi, pj, dist, want, "near_pairs max_dist=0")
    assert strand.dtype == np.uint8 and not strand.any()


def test_near_pairs_beyond_one_launch_one_edit(gpu_api):
    letters, planted, _ = _set()
    pi, pj, dist, strand = gpu_api.near_pairs(_reads(), 1, both_strands=False)
    got = set(zip(pi.tolist(), pj.tolist()))
    print("near_pairs max_dist=1: %d pairs, %d of %d planted" % (len(got), len(got & set(planted)), len(planted)))
    assert len(got) == len(pi) and set(planted) <= got
    text = [row.tobytes().decode() for row in letters[np.unique(np.concatenate([pi, pj]))]]
    at = {int(x): k for k, x in enumerate(np.unique(np.concatenate([pi, pj])).tolist())}
    for i, j, d in zip(pi.tolist(), pj.tolist(), dist.tolist()):
        assert d <= 1 and ref.ed(text[at[i]], text[at[j]]) == d, (i, j, d)


def test_umi_pairs_deep_bucket(gpu_api):
    want = _set()[2]
    pi, pj, dist = gpu_api.umi_pairs(_reads(), 0, 8)
    _assert_exact(pi, pj, dist, want, "umi_pairs max_dist=0 seed_len=8")
