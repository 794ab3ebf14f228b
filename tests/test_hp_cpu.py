"""CPU: the definition of ngsid_hp_runs on hand-built cases (tests/hp_cases.py, expectations derived by hand), and the policy layer ngspeciesid_amd/hp.py - runs / apply,
every rule of call(), and polish() over the oracle-backed reference (tests/hp_reference.py)."""
import numpy as np
import pytest
from ngspeciesid_amd import hp
from ngspeciesid_amd._capi import ReadSet, HP_NBUCKET, HP_OTHER
import hp_cases as hc
from hp_reference import read_runs, hp_reference, check_lists, HpAdapter, NBUCKET, OTHER


def test_constants():
    assert (HP_NBUCKET, HP_OTHER) == (NBUCKET, OTHER) == (17, 16) and hp.MAX_CALL == 14
    import os, re
    head = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ngsid_hp.h")).read()
    assert re.search(r"#define NGSID_HP_NBUCKET\s+17\b", head) and re.search(r"#define NGSID_HP_OTHER\s+16\b", head) and "ngsid_hp_runs(" in head


@pytest.mark.parametrize("case", hc.HAND, ids=[c["name"] for c in hc.HAND])
def test_hand_cases(case):
    """the columns are written by hand and the buckets derived by hand: no aligner, no oracle"""
    hc.check_ops(case)
    centre = np.frombuffer(case["centre"].encode(), dtype=np.uint8); read = np.frombuffer(case["read"].encode(), dtype=np.uint8)
    got = read_runs(hc.ops_array(case["ops"]), read, centre, case["starts"], case["clip"])
    assert got.tolist() == case["buckets"]


def test_hand_cases_with_the_oracle_columns(oracle):
    """the same cases with the strand and the columns the oracle finds, one group of one read each: the histogram is the hand-derived bucket (the three 'neighbours' cases
    share their sequences: the oracle's traceback prefers the diagonal)"""
    for clip in (False, True):
        cases = [c for c in hc.HAND if c["clip"] == clip and not c["name"].startswith("neighbours_gap_")]
        centres = [c["centre"] for c in cases]; rs = ReadSet.from_strings([c["read"] for c in cases])
        run_off = np.concatenate(([0], np.cumsum([len(c["starts"]) for c in cases]))).astype(np.uint64)
        hist, strand = hp_reference(oracle, centres, rs, np.arange(len(cases) + 1, dtype=np.uint64), run_off, [a for c in cases for a in c["starts"]], clip=clip)
        assert (strand == 0).all() and hist[:, 1].sum() == 0
        exp = np.zeros_like(hist[:, 0])
        for j, b in enumerate(b for c in cases for b in c["buckets"]):
            if b >= 0: exp[j, b] = 1
        bad = np.nonzero((hist[:, 0] != exp).any(axis=1))[0]
        assert len(bad) == 0, "runs %s differ" % bad.tolist()


def test_list_checks():
    c = ["ACCCGT", "AAT"]
    assert check_lists(c, [0, 3, 4], [0, 1, 4, 2]) and check_lists(c, [0, 0, 0], [])
    assert not check_lists(c, [0, 1, 1], [2])               # inside the run CCC
    assert not check_lists(c, [0, 2, 2], [4, 1])            # descending
    assert not check_lists(c, [0, 0, 1], [3])               # at the centre length


def test_runs_and_apply_round_trip():
    s = "AACGGGTN" + "T" * 20 + "A"
    st, ln = hp.runs(s)
    assert st.tolist() == [0, 2, 3, 6, 7, 8, 28] and ln.tolist() == [2, 1, 3, 1, 1, 20, 1] and st.dtype == np.uint32
    assert hp.apply(s, st, ln) == s and hp.apply(s, [], []) == s
    t = hp.apply(s, [3, 8], [4, 1])
    assert t == "AACGGGGTNTA"
    st2, ln2 = hp.runs(t)
    assert len(st2) == len(st) and [t[int(a)] for a in st2] == [s[int(a)] for a in st]            # no run lost, none merged, the letters stay
    assert hp.apply(t, [3, 9], [3, 20]) == s
    assert hp.runs("")[0].tolist() == [] and hp.runs("G")[1].tolist() == [1]
    with pytest.raises(ValueError):
        hp.apply(s, [4], [2])                               # not the first base of a run
    with pytest.raises(ValueError):
        hp.apply(s, [3], [0])                               # a run is never removed


def _hist(s0, s1):
    h = np.zeros((1, 2, 17), dtype=np.uint32)
    for s, d in enumerate((s0, s1)):
        for b, n in d.items(): h[0, s, b] = n
    return h


KW = dict(min_depth=8, min_share=0.5, min_margin=0.2, min_strand_depth=4)


def test_call_rules_one_by_one():
    """a histogram every rule passes, then one per rule that this rule alone rejects: relaxing that one threshold calls it"""
    assert hp.call(_hist({4: 6, 3: 1}, {4: 6, 3: 1}), [3], **KW).tolist() == [4]
    assert hp.call(_hist({2: 6, 3: 1}, {2: 6, 3: 1, 16: 30}), [3], **KW).tolist() == [2]          # shorter as well; bucket 16 is no usable depth
    # depth
    h = _hist({4: 3}, {4: 3})
    assert hp.call(h, [3], **KW).tolist() == [3] and hp.call(h, [3], **dict(KW, min_depth=6)).tolist() == [4]
    # share
    h = _hist({4: 5, 3: 1, 5: 3, 2: 2}, {4: 5, 3: 1, 5: 2, 2: 2})
    assert hp.call(h, [3], **KW).tolist() == [3] and hp.call(h, [3], **dict(KW, min_share=0.4)).tolist() == [4]
    # margin over the centre's own length
    h = _hist({4: 6, 3: 5}, {4: 6, 3: 5})
    assert hp.call(h, [3], **KW).tolist() == [3] and hp.call(h, [3], **dict(KW, min_margin=0.05)).tolist() == [4]
    # a strand with depth of its own that prefers the centre's length
    h = _hist({4: 12}, {4: 1, 3: 4})
    assert hp.call(h, [3], **KW).tolist() == [3] and hp.call(h, [3], **dict(KW, min_strand_depth=6)).tolist() == [4]
    # the range 1 .. 14: 15 means "15 or more", 0 would remove the run
    assert hp.call(_hist({15: 6, 14: 1}, {15: 6}), [14], **KW).tolist() == [14] and hp.call(_hist({13: 6, 14: 1}, {13: 6}), [14], **KW).tolist() == [13]
    assert hp.call(_hist({0: 6, 1: 1}, {0: 6}), [1], **KW).tolist() == [1] and hp.call(_hist({2: 6, 1: 1}, {2: 6}), [1], **KW).tolist() == [2]
    assert hp.call(_hist({14: 6}, {14: 6}), [20], **KW).tolist() == [14]                          # a centre run of 15 or more has bucket 15 as its own
    # a tie at the top, the centre's own length as the mode, nothing at all
    assert hp.call(_hist({4: 6, 5: 6}, {}), [3], **KW).tolist() == [3] and hp.call(_hist({3: 9, 4: 2}, {3: 9}), [3], **KW).tolist() == [3]
    assert hp.call(np.zeros((2, 2, 17), np.uint32), [3, 5], **KW).tolist() == [3, 5] and hp.call(np.zeros((0, 2, 17), np.uint32), []).tolist() == []


class _Counting(HpAdapter):
    def __init__(self, oracle):
        super().__init__(oracle); self.calls = []

    def hp_runs(self, centres, *a, **kw):
        self.calls.append(centres.n)
        return super().hp_runs(centres, *a, **kw)


@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(21)
    base = hc.no_repeat(rng, 300)
    truth = hc.with_runs(base, [(60, "A", 4), (130, "C", 6), (131 + 70, "T", 3)])
    truth = "".join(truth)
    st, ln = hp.runs(truth)
    big = [int(a) for a, n in zip(st, ln) if n >= 3]
    assert len(big) == 3
    short = hp.apply(truth, big, [int(n) - 1 for a, n in zip(st, ln) if n >= 3])
    reads = [truth] * 6 + [hc.revcomp(truth)] * 6
    return truth, short, ReadSet.from_strings(reads), [np.arange(12, dtype=np.uint32)]


def test_polish_restores_three_shortened_runs(oracle, planted):
    truth, short, rs, lists = planted
    api = _Counting(oracle)
    seqs, changes = hp.polish(api, [short], rs, lists, k=13, w=20, rounds=2)
    assert seqs == [truth] and len(short) == len(truth) - 3
    assert sorted((c["letter"], c["old"], c["new"], c["round"]) for c in changes[0]) == [("A", 3, 4, 0), ("C", 5, 6, 0), ("T", 2, 3, 0)]
    assert all(c["hist"].shape == (2, 17) and c["hist"][0, c["new"]] == 6 and c["hist"][1, c["new"]] == 6 and c["hist"].sum() == 12 for c in changes[0])
    assert api.calls == [1, 1]                                                                   # the second round sees the changed centre and changes nothing


def test_polish_leaves_a_correct_centre_alone(oracle, planted):
    truth, short, rs, lists = planted
    api = _Counting(oracle)
    seqs, changes = hp.polish(api, [truth, truth[:0]], rs, lists + [np.zeros(0, np.uint32)], k=13, w=20, rounds=2)
    assert seqs == [truth, ""] and changes == [[], []] and api.calls == [1]                      # no second round


def test_a_letter_the_centre_lacks_is_not_a_longer_run(oracle):
    """truth ..AAAGT.., centre ..AAAT..: a vote on the insertion flag alone would write AAAAT"""
    rng = np.random.default_rng(22)
    left, right = hc.no_repeat(rng, 120), hc.no_repeat(rng, 120)
    left = left[:-1] + "C"; right = "T" + hc.no_repeat(rng, 119, first_not="T")
    truth = left + "AAAG" + right; centre = left + "AAA" + right
    rs = ReadSet.from_strings([truth] * 8 + [hc.revcomp(truth)] * 8)
    api = _Counting(oracle)
    seqs, changes = hp.polish(api, [centre], rs, [np.arange(16, dtype=np.uint32)], k=13, w=20)
    assert seqs == [centre] and changes == [[]] and api.calls == [1]
    st, _ = hp.runs(centre)
    hist, _ = api.hp_runs(ReadSet.from_strings([centre]), rs, [0, 16], [0, len(st)], st)
    at = st.tolist().index(120)
    assert hist[at, :, 16].tolist() == [8, 8] and hist[at, :, :16].sum() == 0
