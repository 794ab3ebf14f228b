"""The pigeonhole rule and the search of csrc/k_umi.hip on Python ints (tests/umi_seed_model.py) against brute force (tests/umi_reference.py): keys, shifts, the
smaller-index rule, the first-witness dedupe, the Myers column and the short path, for every max_dist and seed_len of the header.  No device."""
import os
import numpy as np
import pytest
import variants_reference as vr
import variants_cases as vc
import umi_reference as ur
import umi_cases as uc
import umi_seed_model as sm


def test_constants_are_the_headers():
    from ngspeciesid_amd._capi import UMI_MAX_LEN, UMI_MAX_DIST
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "ngsid_umi.h")).read()
    assert "#define NGSID_UMI_MAX_LEN   %d " % UMI_MAX_LEN in text and "#define NGSID_UMI_MAX_DIST   %d\n" % UMI_MAX_DIST in text
    assert (UMI_MAX_LEN, UMI_MAX_DIST) == (64, 8)


def _has_witness(a, b, d, g):
    """some seed j of a occurs exactly in b at j g + s, |s| <= d"""
    for j in range(d + 1):
        seed = a[j * g:(j + 1) * g]
        for s in range(-d, d + 1):
            p = j * g + s
            if p >= 0 and p + g <= len(b) and b[p:p + g] == seed: return True
    return False


@pytest.mark.parametrize("d", range(0, 5))
def test_the_rule_misses_no_pair_within_d(d):
    """random pairs within d of a seedable sequence: a witness always exists"""
    rng = np.random.default_rng(100 + d)
    checked = 0
    for g in (4, 6, 9):
        need = (d + 1) * g
        if need > 64: continue
        for _ in range(250):
            a = vc.rand_seq(rng, int(rng.integers(need, 65)), "ACGTN")
            b = a
            for _ in range(int(rng.integers(0, d + 1))): b = uc.one_edit(rng, b) if b else b
            if vr.ed(a, b) <= d and len(b) <= 64:
                assert _has_witness(a, b, d, g), (a, b, d, g)
                checked += 1
    assert checked > 300


@pytest.mark.parametrize("d", (0, 1, 3, 8))
def test_column_is_the_edit_distance(d):
    rng = np.random.default_rng(7 + d)
    cases = [("", ""), ("", "ACG"[:min(d, 3)]), ("A", ""), ("N", "N"), ("N", "A"), ("A" * 64, "A" * 64), ("A" * 64, "A" * 63), ("AC" * 32, "CA" * 32)]
    for L in (1, 2, 17, 36, 63, 64):
        for _ in range(12):
            a = vc.rand_seq(rng, L, "ACGTN"); b = a
            for _ in range(int(rng.integers(0, d + 3))): b = uc.one_edit(rng, b) if b else "A"
            cases.append((a, b[:64]))
        cases.append((vc.rand_seq(rng, L), vc.rand_seq(rng, L)))
    for a, b in cases:
        for x, y in ((a, b), (b, a)):
            want = vr.ed(x, y)
            assert sm.column_ed(sm.planes(x), len(x), sm.planes(y), len(y), d) == (want if want <= d else -1), (x, y, d)


@pytest.mark.parametrize("d,g", [(d, g) for d in range(0, 9) for g in (4, 5, 9, 16)] + [(3, g) for g in (6, 7, 8, 10, 11, 12, 13, 14, 15)])
def test_search_equals_brute_force_and_verifies_each_pair_once(d, g):
    rng = np.random.default_rng(1000 * d + g)
    seqs = uc.search_set(rng, d, g)[:90]
    found, verified, candidates = sm.search(seqs, d, g)
    assert found == ur.pairs(seqs, d)
    assert len(set(verified)) == len(verified), "a pair went through the column twice"
    assert all(a < b for a, b in verified)


def test_dedupe_family_and_identical_sequences():
    """a family that matches in every seed and at several shifts (a low-complexity sequence): many candidate entries, one verification per pair"""
    seqs = ["ACACACACACACACACACACACACACACACACACAC"] * 5 + ["ACACACACACACACACACACACACACACACACACACAC", "CACACACACACACACACACACACACACACACACA"]
    for d, g in ((3, 9), (2, 4), (1, 16)):
        found, verified, candidates = sm.search(seqs, d, g)
        assert found == ur.pairs(seqs, d) and len(found) >= 10
        assert len(set(verified)) == len(verified) and {(i, j) for i, j, _ in found} <= set(verified)
        assert candidates > 3 * len(verified)


def test_everything_short():
    """seed_len 16 at max_dist 8 needs 144 letters: no sequence is seedable and every pair goes down the short path"""
    rng = np.random.default_rng(3)
    seqs = uc.search_set(rng, 8, 16)[:60]
    found, verified, candidates = sm.search(seqs, 8, 16)
    assert candidates == 0 and found == ur.pairs(seqs, 8)


def test_result_does_not_depend_on_seed_len():
    rng = np.random.default_rng(9)
    seqs, _ = vc.families(rng, 6, 8, 36, 0.05)
    want = ur.pairs(seqs, 3)
    assert len(want) > 20
    for g in range(4, 17):
        assert sm.search(seqs, 3, g)[0] == want, g
