"""The W-word band recurrence of csrc/k_near.hip, as the Python-int model of variants_band_model.py, against the full DP of variants_reference.py, for W = 1, 2, 4
and 8.  CPU only."""
import itertools
import numpy as np
import pytest
import variants_band_model as bm
import variants_reference as ref
import variants_cases as vc

WS = (1, 2, 4, 8)
SMALLEST_K = {1: 0, 2: 32, 4: 64, 8: 128}      # the smallest bound that selects each W
WIDE_K = (32, 63, 64, 127, 128, 255)            # the smallest and the largest bound of W = 2, 4, 8; a test parametrised by K runs the band that K selects


def _run(a, b, K, W, info=None):
    return bm.band_ed(bm.pack_wide(a), bm.pack(b, bm.TEXT), len(a), len(b), K, W, info)


def _want(a, b, K):
    d = ref.ed(a, b)
    return d if d <= K else -1


def test_widths_and_their_bounds():
    assert [bm.edits(W) for W in WS] == [31, 63, 127, 255] and bm.WIDTHS == WS
    assert [bm.width_for(K) for K in (0, 31, 32, 63, 64, 127, 128, 255)] == [1, 1, 2, 2, 4, 4, 8, 8]
    assert all(bm.width_for(SMALLEST_K[W]) == W and bm.width_for(bm.edits(W)) == W for W in WS)
    with pytest.raises(ValueError):
        bm.width_for(256)


def _every_small_pair(W):
    strs = ["".join(t) for n in range(7) for t in itertools.product("AC", repeat=n)]
    packs = {s: (bm.pack_wide(s), bm.pack(s, bm.TEXT)) for s in strs}
    for a in strs:
        for b in strs:
            d = ref.ed(a, b)
            for K in range(4):
                info = {}
                got = bm.band_ed(packs[a][0], packs[b][1], len(a), len(b), K, W, info)
                assert got == (d if d <= K else -1), (a, b, K, W, got, d)
                if d <= K: assert info["dead_at"] is None, (a, b, K, W, info)


def test_every_small_pair():
    """every pair of strings over {A, C} up to length 6, K = 0 .. 3, one band word: the value, -1 beyond K, and no pair within K ever declared dead"""
    _every_small_pair(1)


@pytest.mark.parametrize("W", WS[1:])
def test_every_small_pair_of_width(W):
    """the same pairs and bounds on 2, 4 and 8 band words"""
    _every_small_pair(W)


@pytest.mark.parametrize("K", (0, 1, 2, 15, 30, 31) + WIDE_K)
def test_border_lengths(K):
    """random and related pairs at the lengths where the band, the word loads and the virtual rows change shape, and 650; the early exit as a property: the result
    is -1 iff the full DP's distance exceeds K; the farthest pattern word read stays below read_bound() and that inside the planes"""
    W = bm.width_for(K)
    rng = np.random.default_rng(100 + K)
    L = vc.LENGTHS(K) + [650]
    n_alive = n_dead = 0
    for la in L:
        for lb in L:
            pairs = [(vc.rand_seq(rng, la), vc.rand_seq(rng, lb))] if max(la, lb) <= 129 else []
            if abs(la - lb) <= K + 2:
                left = max(K - abs(la - lb), 0)
                pairs += [vc.related_pair(rng, la, lb, e) for e in (0, left, 3, left + 3)]
            for a, b in pairs:
                info = {}
                got = _run(a, b, K, W, info)
                d = ref.ed(a, b)
                assert (got == -1) == (d > K), (la, lb, K, W, got, d)
                assert got == (d if d <= K else -1), (la, lb, K, W, got, d)
                if d <= K:
                    n_alive += 1
                    assert info["dead_at"] is None and info["columns"] == lb
                else:
                    n_dead += 1
                assert all(x <= y for x, y in zip(info["diag"], info["diag"][1:])), "the tracked diagonal decreased"
                if lb: assert info["far"] <= bm.read_bound(la, lb, W) < bm.n_words_wide(la)
    assert n_alive >= len(L) and n_dead >= 4


@pytest.mark.parametrize("W", WS)
def test_poly_a_carries_cross_every_word(W):
    """poly-A against poly-A, longer than the band: the sum (Eq & VP) + VP carries through every word of every column (one word: there is no word to carry into)"""
    B, K = 64 * W, 32 * W - 1
    n = B + 70
    for diff in (0, 1, K, K + 1):
        a, b = "A" * n, "A" * (n + diff)
        for x, y in ((a, b), (b, a)):
            info = {}
            assert _run(x, y, K, W, info) == (diff if diff <= K else -1), (W, diff)
            if diff <= K and W > 1: assert info["carries"] >= len(y) - B, (W, diff, info["carries"])
            if W == 1: assert info["carries"] == 0
    g = "A" * (n // 2) + "G" + "A" * (n - n // 2 - 1)
    assert _run("A" * n, g, K, W) == 1 and _run(g, "A" * n, K, W) == 1 and _run(g, g, 0, W) == 0
    assert _run("A" * n, g, 0, W) == -1


@pytest.mark.parametrize("K", (1, 15, 31) + WIDE_K)
def test_outermost_diagonals_and_exact_distance(K):
    """indel-only pairs whose path runs along the outermost band diagonal, both ways round; pairs at exactly K and exactly K + 1"""
    W = bm.width_for(K)
    rng = np.random.default_rng(7 + K)
    for n in sorted({K, K + 2, 64, 129, 300}):
        for where in ("lead", "trail", "mid"):
            a, b = vc.indel_only(rng, n, K, where)
            for x, y in ((a, b), (b, a)):
                assert _run(x, y, K, W) == K, (n, where, K, W)
                assert _run(x, y, K - 1, W) == -1
        if n >= K + 1:
            for k in (K, K + 1):
                a, b = vc.at_distance(rng, n, k)
                assert ref.ed(a, b) == k
                info = {}
                assert _run(a, b, K, W, info) == (k if k <= K else -1), (n, k, K, W)
                assert (info["dead_at"] is None) == (k <= K)


def _strands_and_letters(W):
    rng = np.random.default_rng(3)
    for n in (1, 31, 64, 97):
        a = vc.rand_seq(rng, n, "ACGTN")
        b = vc.mutate(rng, a, 0.05)
        for K in sorted({3, 31, 32 * W - 1}):
            for x, y in ((a, b), (a, ref.rc(b)), (b, ref.rc(a))):
                d, s = ref.D(x, y)
                assert bm.ed_within(x, y, K, W) == ((d, s) if d <= K else (-1, 0)), (n, K, W)
                assert bm.ed_within(x, y, K, W, both_strands=False)[0] == _want(x, y, K)
                if K <= 31: assert bm.ed_within(x, y, K, W) == bm.ed_within(x, y, K, 1)
    assert bm.ed_within("ANNA", "ANNA", 2, W) == (0, 0)
    assert bm.ed_within("ANNA", "AAAA", 2, W, both_strands=False) == (2, 0)
    assert bm.ed_within("N", "A", 1, W, both_strands=False) == (1, 0)
    pal = "ACGTTAACGT"
    assert ref.rc(pal) == pal and bm.ed_within(pal, pal, 5, W) == (0, 0)
    assert bm.ed_within("AAAAC", "GTTTT", 3, W) == (0, 1)
    assert bm.ed_within("", "", 0, W) == (0, 0) and bm.ed_within("", "ACG", 3, W) == (3, 0) and bm.ed_within("ACG", "", 2, W) == (-1, 0)


def test_strands_and_letters():
    """the reverse-complement text variant, the tie rule, N against N and N against A, a reverse-complement palindrome, empty sequences, on one band word"""
    _strands_and_letters(1)


@pytest.mark.parametrize("W", WS[1:])
def test_strands_letters_and_what_one_word_gives(W):
    """the same on 2, 4 and 8 band words; below 32 edits every W gives what W = 1 gives"""
    _strands_and_letters(W)


def test_layout_bounds_of_every_width():
    """the loop never reads a word beyond the planes: the farthest reads are the pattern word loaded ahead in the last block, with n <= m + 32 W - 1, and text
    word ((n - 1) >> 5) + 1"""
    for W in WS:
        for m in list(range(0, 300)) + [16383, 16384]:
            n = m + 32 * W - 1
            assert bm.read_bound(m, n, W) < bm.n_words_wide(m)
            assert ((n - 1) >> 5) + 1 < bm.n_words(n)
