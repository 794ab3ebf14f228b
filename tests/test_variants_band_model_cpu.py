"""The one-word band recurrence of csrc/k_near.hip, as the Python-int model of variants_band_model.py, against the full DP of variants_reference.py.  CPU only."""
import itertools
import numpy as np
import pytest
import variants_band_model as bm
import variants_reference as ref
import variants_cases as vc


def _want(a, b, K):
    d = ref.ed(a, b)
    return d if d <= K else -1


def _strings(alphabet, max_len):
    for n in range(max_len + 1):
        for t in itertools.product(alphabet, repeat=n):
            yield "".join(t)


def test_every_small_pair():
    """every pair of strings over {A, C} up to length 6, K = 0 .. 3: the value, -1 beyond K, and no pair within K ever declared dead"""
    strs = list(_strings("AC", 6))
    packs = {s: (bm.pack(s, bm.PATTERN), bm.pack(s, bm.TEXT)) for s in strs}
    full = {(a, b): ref.ed(a, b) for a in strs for b in strs}
    for K in range(4):
        for a in strs:
            for b in strs:
                info = {}
                got = bm.band_ed(packs[a][0], packs[b][1], len(a), len(b), K, info)
                d = full[(a, b)]
                assert got == (d if d <= K else -1), (a, b, K, got, d)
                if d <= K: assert info["dead_at"] is None, (a, b, K, info)


@pytest.mark.parametrize("K", [0, 1, 2, 15, 30, 31])
def test_border_lengths(K):
    """random and related pairs at the lengths where the band, the word loads and the virtual rows change shape"""
    rng = np.random.default_rng(100 + K)
    L = vc.LENGTHS(K)
    n_alive = 0
    for la in L:
        for lb in L:
            pairs = [(vc.rand_seq(rng, la), vc.rand_seq(rng, lb))]
            if abs(la - lb) <= K + 2:
                pairs += [vc.related_pair(rng, la, lb, e) for e in (0, max(K - abs(la - lb), 0), 3)]
            for a, b in pairs:
                info = {}
                got = bm.band_ed(bm.pack(a, bm.PATTERN), bm.pack(b, bm.TEXT), la, lb, K, info)
                d = ref.ed(a, b)
                assert got == (d if d <= K else -1), (la, lb, K, got, d)
                if d <= K:
                    n_alive += 1
                    assert info["dead_at"] is None and info["columns"] == lb
                assert all(x <= y for x, y in zip(info["diag"], info["diag"][1:])), "the tracked diagonal decreased"
    assert n_alive >= len(L)


@pytest.mark.parametrize("K", [1, 15, 31])
def test_outermost_diagonals_and_exact_distance(K):
    """indel-only pairs whose path runs along the outermost band diagonal, both ways round; pairs at exactly K and exactly K + 1"""
    rng = np.random.default_rng(7 + K)
    for n in (K, 64, 129, 300):
        for where in ("lead", "trail", "mid"):
            a, b = vc.indel_only(rng, n, K, where)
            for x, y in ((a, b), (b, a)):
                assert bm.band_ed(bm.pack(x, bm.PATTERN), bm.pack(y, bm.TEXT), len(x), len(y), K) == K, (n, where)
                assert bm.band_ed(bm.pack(x, bm.PATTERN), bm.pack(y, bm.TEXT), len(x), len(y), K - 1) == -1
        if n >= 8 * (K + 1) or n == 300:
            for k in (K, K + 1):
                a, b = vc.at_distance(rng, n, k)
                assert ref.ed(a, b) == k
                assert bm.band_ed(bm.pack(a, bm.PATTERN), bm.pack(b, bm.TEXT), n, n, K) == (k if k <= K else -1)


def test_strands_and_letters():
    """the reverse-complement text variant, the tie rule, N against N and N against A, a reverse-complement palindrome"""
    rng = np.random.default_rng(3)
    for n in (1, 31, 64, 97):
        a = vc.rand_seq(rng, n, "ACGTN")
        b = vc.mutate(rng, a, 0.05)
        for K in (3, 31):
            for x, y in ((a, b), (a, ref.rc(b)), (b, ref.rc(a))):
                d, s = ref.D(x, y)
                assert bm.ed_within(x, y, K) == ((d, s) if d <= K else (-1, 0)), (n, K)
                assert bm.ed_within(x, y, K, both_strands=False)[0] == _want(x, y, K)
    assert bm.ed_within("ANNA", "ANNA", 2) == (0, 0)
    assert bm.ed_within("ANNA", "AAAA", 2, both_strands=False) == (2, 0)
    assert bm.ed_within("N", "A", 1, both_strands=False) == (1, 0)
    pal = "ACGTTAACGT"
    assert ref.rc(pal) == pal and bm.ed_within(pal, pal, 5) == (0, 0)
    assert bm.ed_within("AAAAC", "GTTTT", 3) == (0, 1)
    assert bm.ed_within("", "", 0) == (0, 0) and bm.ed_within("", "ACG", 3) == (3, 0) and bm.ed_within("ACG", "", 2) == (-1, 0)


def test_layout_bounds():
    """the loop never reads a word beyond n_words(): the farthest reads are pattern word ((n - 1) >> 5) + 2 with n <= m + 31, and text word (n - 1) >> 5"""
    for m in list(range(0, 200)) + [16384]:
        n = m + 31
        assert ((n - 1) >> 5) + 2 < bm.n_words(m)
        assert ((n - 1) >> 5) < bm.n_words(n)
