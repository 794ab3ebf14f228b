"""CPU: the plain reference of the ngsid_ed_align_batch contract (ed_reference.py) against a scalar triple loop and the hand-made answers, the
oracle against the reference on every edge family of ed_cases.py (distance, span and break points, exactly), and the conditions that make a
family what it claims to be - asserted on the reference's results."""
import numpy as np
import pytest
from ngspeciesid_amd._capi import ReadSet
import ed_cases
import ed_reference as ref

FAMILIES = list("abcdefg")


def test_vectorised_rows_equal_the_scalar_triple_loop():
    rng = np.random.default_rng(17)
    letters = "ACGT" * 6 + "acgt" + "NnRY"
    qs, ts = [], []
    for k in range(300):
        n = 0 if k % 37 == 0 else int(rng.integers(1, 41)); m = 0 if k % 41 == 0 else int(rng.integers(1, 41))
        t = "".join(letters[x] for x in rng.integers(0, len(letters), m))
        if k % 3 == 0 and m:                                   # related: a mutated slice, so that the paths are not all mismatch runs
            a = int(rng.integers(0, m)); q = list(t[a:a + n])
            for x in range(len(q)):
                u = rng.random()
                if u < 0.1: q[x] = ""
                elif u < 0.2: q[x] += "ACGT"[rng.integers(0, 4)]
                elif u < 0.3: q[x] = "ACGTN"[rng.integers(0, 5)]
            q = "".join(q)[:40]
        else:
            q = "".join(letters[x] for x in rng.integers(0, len(letters), n))
        if k % 5 == 0: q, t = q[:12] * 3, (t[:5] + q[:12] * 3)[:40]      # repeats: ties in the last row and between moves
        qs.append(q); ts.append(t)
    assert sum(1 for q in qs if not q) >= 5 and sum(1 for t in ts if not t) >= 5
    idx = np.arange(300)
    for W, nw in ((7, 6), (1, 40), (64, 2)):
        d, span, bp = ref.ed_align_batch(qs, ts, idx, idx, window=W, bp_windows=nw)
        for p in range(300):
            ed, es, eb = ref.scalar_outputs(qs[p], ts[p], W, nw)
            assert d[p] == ed and span[p].tolist() == es and bp[p].tolist() == eb, (qs[p], ts[p], W, nw)


def test_reference_reproduces_the_hand_made_answers():
    """the expectations of test_ed_oracle.py::test_known_answers, on the reference"""
    q = ["ACGTACGTTTGA", "ACGT", "", "ACNT", "acgt"]; t = ["TTTACGTACGTTGATTT", "ACGT", "GGACGTGG"]
    d, span, bp = ref.ed_align_batch(q, t, [0, 1, 2, 3, 4, 1], [0, 1, 0, 1, 1, 2], window=5, bp_windows=4)
    assert list(d) == [1, 0, 0, 1, 0, 0]
    assert list(span[0]) == [0, 11, 3, 13]
    assert list(span[1]) == [0, 3, 0, 3]
    assert list(span[2]) == [-1, -1, -1, -1]
    assert list(span[5]) == [0, 3, 2, 5]
    assert bp[0].tolist() == [[0, 1, 3, 4], [2, 6, 5, 9], [8, 11, 10, 13], [-1, -1, -1, -1]]
    assert list(d[3:5]) == [1, 0]
    assert bp[2].tolist() == [[-1] * 4] * 4


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_equals_reference(oracle, family):
    for case in ed_cases.cases(family):
        exp = ref.case_results(case)
        Q = ReadSet.from_strings(case.queries); T = ReadSet.from_strings(case.targets)
        # the oracle has no state across pairs and runs one full DP for each: it gets every distinct pair once, at its first position in the call
        _, at = np.unique(case.q_idx.astype(np.int64) << 32 | case.t_idx, return_index=True); at.sort()
        got = oracle.ed_align_batch(Q, T, case.q_idx[at], case.t_idx[at], window=case.window, bp_windows=case.bp_windows)
        for nm, a, b in zip(["distance", "span", "bp"], got, exp):
            bad = np.nonzero((a != b[at]).reshape(len(at), -1).any(axis=1))[0]
            if len(bad):
                p = int(at[bad[0]]); a = a[None, bad[0]].repeat(p + 1, axis=0); q = case.queries[case.q_idx[p]]; t = case.targets[case.t_idx[p]]
                pytest.fail("%s: %s of pair %d (n %d, m %d, reference distance %d, tag %s) oracle %s reference %s"
                            % (case.name, nm, p, len(q), len(t), exp[0][p], case.tags[p], a[p].ravel()[:16], b[p].ravel()[:16]))


# ---- family conditions: a family must not claim coverage it does not have
def _nm(case):
    n = np.array([len(x) for x in case.queries])[case.q_idx]; m = np.array([len(x) for x in case.targets])[case.t_idx]
    return n, m


def test_family_a_has_every_named_length():
    qn, tm, deltas = set(), set(), set()
    for case in ed_cases.cases("a"):
        n, m = _nm(case)
        qn |= set(n.tolist()); tm |= set(m.tolist())
        deltas |= {tag[2] for tag in case.tags if tag[0] == "near"}
        assert (n.max() > 1024) == (case.name == "a_gt1024")
    assert qn == set(ed_cases.A_QLENS) and {0, 1, 63, 64, 65} <= tm and deltas == set(range(-9, 10))


def test_family_b_has_each_distance_around_each_band_in_each_construction():
    cs = ed_cases.cases("b")
    assert [c.name for c in cs] == ["b_K%d" % K for K in ed_cases.B_KS]
    for K, case in zip(ed_cases.B_KS, cs):
        d = ref.case_results(case)[0]; n, m = _nm(case)
        for constr in ("spread", "qblock", "tblock"):
            sel = np.array([tag[0] == constr for tag in case.tags])
            have = set(d[sel].tolist())
            assert {K - 1, K, K + 1} <= have, (K, constr, sorted(have))
        assert (d >= 2 * K - K // 8).any()             # "about 2K" (a block of 2K between flanks the instance has room for comes out cheaper: the flank is clipped)
        for want in (K - 1, K, K + 1):
            assert ((d == want) & (n > m)).any() and ((d == want) & (n < m)).any(), (K, want)
        # every distinct pair also fills a bundle of its own
        key = case.q_idx.astype(np.int64) * 100000 + case.t_idx
        for b0 in range(64, len(key), 64): assert len(set(key[b0:b0 + 64].tolist())) == 1
        assert len(set(key[:64].tolist())) == len(set(key.tolist()))
    # the instance each call aims at
    assert [max(len(q) for q in c.queries) for c in cs][:4] <= [256, 512, 768, 1024] and max(len(q) for q in cs[4].queries) > 1024
    assert max(len(q) for q in cs[1].queries) > 256 and max(len(q) for q in cs[2].queries) > 512 and max(len(q) for q in cs[3].queries) > 768


def test_family_c_bundles_mix_the_extremes():
    cs = ed_cases.cases("c")
    assert sorted({len(c.q_idx) for c in cs}) == [1, 63, 64, 65, 129]
    for case in cs:
        n, m = _nm(case)
        if len(n) >= 63:
            for b0 in range(0, len(n) - 62, 64):
                dn = (n - m)[b0:b0 + 64]
                assert dn.min() <= -1000 and dn.max() >= 150, case.name
                assert (n[b0:b0 + 64] >= 700).sum() >= 40
        if len(n) >= 64:
            assert (n[:64] == 0).any() and (m[:64] == 0).any() and (n[:64] == 1).any()
            assert len(set(case.q_idx.tolist())) < len(case.q_idx)                      # repeated, non-identity indices
            assert not np.array_equal(case.q_idx, np.arange(len(case.q_idx)))
    by = {c.name: c for c in cs}
    n0, _ = _nm(by["c_lane0_top1000"]); n63, _ = _nm(by["c_lane63_top1000"])
    assert n0[0] == 0 and n63[63] == 0
    assert max(len(q) for q in by["c_lane0_top1000"].queries) <= 1024 < max(len(q) for q in by["c_lane0_top1100"].queries)


def test_family_d_has_ties_in_the_last_row():
    case, = ed_cases.cases("d")
    tied = 0
    for p in range(len(case.q_idx)):
        q, t = case.queries[case.q_idx[p]], case.targets[case.t_idx[p]]
        if 0 < len(q) <= 200:
            row = ref.last_row(q, t)
            tied += int((row == row.min()).sum() >= 2)
    assert tied >= 5
    d, span, _ = ref.case_results(case)
    copies = [p for p, tag in enumerate(case.tags) if tag == "exact_copies"]
    for p in copies:                                                                    # the leftmost copy wins
        q, t = case.queries[case.q_idx[p]], case.targets[case.t_idx[p]]
        assert d[p] == 0 and span[p][2] == t.find(q) and t.count(q) >= 3
    alln = [p for p, tag in enumerate(case.tags) if tag == "all_N"]
    assert alln and all(d[p] == len(case.queries[case.q_idx[p]]) for p in alln)


def test_family_e_has_an_empty_window_between_aligned_ones():
    cs = ed_cases.cases("e")
    assert {c.window for c in cs} == set(ed_cases.E_WINDOWS)
    inner = {}
    for case in cs:
        nwin = (max(len(t) for t in case.targets) + case.window - 1) // case.window
        kind = "fewer" if case.bp_windows < nwin else "equal" if case.bp_windows == nwin else "more"
        assert case.name.endswith(kind)
        bp = ref.case_results(case)[2]
        for p in range(len(bp)):
            full = np.nonzero(bp[p, :, 0] >= 0)[0]
            if len(full) >= 2 and (bp[p, full[0]:full[-1], 0] < 0).any(): inner[case.window] = inner.get(case.window, 0) + 1
    assert all(inner.get(W, 0) >= 1 for W in (7, 64, 100, 500)), inner
    # alignments that start and end exactly on a window boundary
    case = [c for c in cs if c.name == "e_w100_equal"][0]
    d, span, bp = ref.case_results(case)
    p = case.tags.index(("slice", 100, 300))
    assert d[p] == 0 and span[p].tolist() == [0, 199, 100, 299] and bp[p, 0].tolist() == [-1] * 4 and bp[p, 1].tolist() == [0, 99, 100, 199] and bp[p, 3].tolist() == [-1] * 4


def test_family_f_has_the_named_lengths_at_low_error():
    cs = ed_cases.cases("f")
    for n, case in zip(ed_cases.F_QLENS, cs):
        d = ref.case_results(case)[0]; qn, _ = _nm(case)
        assert (qn == n).all() and 0.002 * n <= d[0] <= 0.04 * n, (n, d[0])
    qn, tm = _nm(cs[-1])
    assert cs[-1].name == "f_mixed" and len(qn) > 64 and (qn[:64] - tm[:64]).min() < -2000 and (qn[:64] > 2000).any()


def test_family_g_has_its_classes_and_both_sides_of_180():
    cs = {c.name: c for c in ed_cases.cases("g")}
    assert len(cs["g_4096"].q_idx) == 4096 and len(cs["g_4097"].q_idx) == 4097
    empty = {"g_4096": None, "g_4097": None, "g_no_513_768": 2, "g_no_769_896": 3, "g_no_gt896": 4, "g_top1100": None}
    for name, case in cs.items():
        n, _ = _nm(case); d = ref.case_results(case)[0]
        assert len(n) >= 4096 and len(set(zip(case.q_idx.tolist(), case.t_idx.tolist()))) <= 62
        for c, (lo, hi) in enumerate(ed_cases.G_CLASSES):
            cnt = int(((n >= lo) & (n <= (hi if c < 4 else 1 << 30))).sum())
            assert (cnt == 0) == (empty[name] == c), (name, c, cnt)
        band = 64 + int(n.max()) // 32                                                  # the default band of the call
        assert (d < band).any() and ((d > band) & (d <= 180)).any() and (d > 180).any(), name
    assert _nm(cs["g_top1100"])[0].max() == 1100 and _nm(cs["g_4096"])[0].max() == 1024
