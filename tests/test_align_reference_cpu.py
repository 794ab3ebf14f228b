"""CPU: the plain reference of the sg_align contract (align_reference.py) against the textbook Gotoh score, its own re-scored columns and hand-worked answers;
the oracle against the reference on EVERY pair of the edge families of align_cases.py (score, columns, n_cols, n_match, region - this pins the oracle's
traceback at real shapes); the sensitivity of family c to each of the oracle's alternative tie-break orders; and the conditions that make a family what it
claims to be - asserted on the reference's results and on the lengths, never assumed."""
import ctypes as C
import os
import re
import numpy as np
import pytest
from ngspeciesid_amd._capi import ReadSet
import align_cases as ac
import align_reference as ref
import polish_reference as pref
import textbook_gotoh as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngspeciesid_amd", "csrc")
FAMILIES = list("abcdefg")
CELL_CAP = 250_000_000
# (match, mismatch, open, ext)
SCHEMES = [(2, -2, 3, 1), (4, -8, 16, 4), (2, -2, 3, 0), (2, -2, 1, 3), (2, -2, 2, 2), (1, -3, 2, 2)]


def _src(name):
    with open(os.path.join(CSRC, name)) as f: return f.read()


def test_constants_of_the_builders_are_those_of_the_sources():
    k = _src("k_align.hip")
    m = re.search(r"kAlignClass\[NCLS\] = \{(.*?)\};", k)
    cls = [tuple(int(x.strip().rstrip("u"), 0) for x in g.split(",")) for g in re.findall(r"\{([^{}]*)\}", m.group(1))]
    assert tuple((b, 2 * rp, r) for b, rp, r, _ in cls) == ac.CLASSES
    rpl = [(int(a), int(b)) for a, b in re.findall(r"if \(max_qlen <= (\d+)\) return launch_rpl<(\d+)>", k)]
    last = re.findall(r"\n    return launch_rpl<(\d+)>\(ctx, job, max_qlen, max_tlen\);", k)
    assert tuple(rpl) + ((0xffffffff, int(last[0])),) == ac.RPL32
    assert "job.npairs >= %d && q16 > %d" % (ac.PARTITION_MIN_PAIRS, ac.CLASSES[0][0]) in k
    assert "const int STRIP = 64 * RPL;" in k and "STRIP = 64 * RPL" in _src("k_align16.hip") and "int i0 = lane * R;" in _src("k_align16p.hip")
    assert re.search(r"#define NGSID_ALIGN16_MAXLEN (\d+)u", _src("ngsid_internal.h")).group(1) == str(ac.ALIGN16_MAXLEN)
    common = _src("k_align_common.h")
    assert "#define NEG16 (%d)" % ac.NEG16 in common
    assert "%d steps x %d lanes" % (ac.WALK_STEPS, ac.WALK_LANES) in common
    assert 'job.k > 64' in k
    # the two host predicates, restated in align_cases, at the corner and one step outside each bound
    assert ac.align16_applicable(4, -8, 4, 16, 4000, 4000)
    for bad in ((5, -8, 4, 16, 4000, 4000), (4, -9, 4, 16, 4000, 4000), (4, 1, 4, 16, 4000, 4000), (4, -8, 5, 16, 4000, 4000), (4, -8, 4, 17, 4000, 4000), (4, -8, 4, 16, 4001, 10), (4, -8, 4, 16, 10, 4001)):
        assert not ac.align16_applicable(*bad)
    assert re.search(r"max_qlen <= NGSID_ALIGN16_MAXLEN && max_tlen <= NGSID_ALIGN16_MAXLEN && job.match >= 0 && job.match <= 4 && job.mismatch <= 0 && job.mismatch >= -8 &&\s+job.ext >= 0 && job.ext <= 4 && max_open >= 0 && max_open <= 16;", k)
    assert "return -(long long)(NEG16) + ext + open + match * (qlen < tlen ? qlen : tlen) + (skew ? (qlen + tlen + 1) * ext : 0);" in common


def _small_pairs(seed, count, hi=70):
    rng = np.random.default_rng(seed)
    letters = "ACGT" * 6 + "acgt" + "NnRY"
    out = []
    for x in range(count):
        n = 0 if x % 37 == 5 else int(rng.integers(1, hi + 1)); m = 0 if x % 41 == 7 else int(rng.integers(1, hi + 1))
        t = "".join(letters[y] for y in rng.integers(0, len(letters), m))
        if x % 3 == 0 and m:
            a = int(rng.integers(0, m)); q = ac.mutate(rng, t[a:a + n].upper().replace("R", "A").replace("Y", "C").replace("N", "G"), 0.2)[:hi]
        elif x % 3 == 1: q = ac.hp_rich(rng, n); t = ac.hp_rich(rng, m)
        else: q = "".join(letters[y] for y in rng.integers(0, len(letters), n))
        if x % 5 == 0: u = ac.rseq(rng, 1 + x % 6); q = (u * hi)[:n]; t = (u * hi)[:m]
        out.append((q, t))
    return out


@pytest.mark.parametrize("scheme", SCHEMES, ids=lambda s: "%d/%d/open%d/ext%d" % s)
def test_reference_score_equals_textbook_gotoh_and_its_columns_rescore(scheme):
    """the score against the three-state textbook DP where that is defined (open >= ext), and under every scheme the reference's own columns, re-scored
    independently, consume both sequences, agree with the raw characters and reach the score"""
    ma, mi, op, ex = scheme
    for q, t in _small_pairs(11, 150):
        r = ref.align_pair(q, t, ma, mi, op, ex)
        if op >= ex: assert r.score == tg.gotoh_semiglobal_score(q, t, ma, mi, op, ex), (q, t, scheme)
        # (the recurrences may open a gap again in every column, so with open < ext a further gap column costs open; and an alignment without a diagonal column is
        # one paid gap column between the two free end-gap runs, which the re-scorer cannot tell from them)
        if "=" in r.cols or "X" in r.cols: assert tg.score_of_alignment(q, t, r.cols, ma, mi, op, min(op, ex)) == r.score, (q, t, scheme, r.cols)
        else: assert r.score <= 0
        assert r.n_cols == len(r.cols) and r.n_match == r.cols.count("=")
        diag = [x for x, c in enumerate(r.cols) if c in "=X"]
        if diag:
            first, last = diag[0], diag[-1]
            q_first = r.cols[:first].count("I"); t_first = r.cols[:first].count("D")
            q_last = sum(1 for c in r.cols[:last] if c in "=XI"); t_last = sum(1 for c in r.cols[:last] if c in "=XD")
            assert r.span == (q_first, q_last, t_first, t_last), (q, t, r.cols, r.span)
        else: assert r.span == (-1, -1, -1, -1)


# (query, target, match, mismatch, open, ext, score, columns): worked by hand, one per rule
HAND = [
    # end cell: the FIRST maximum of the last row (lowest column) - AA ends at column 2, the rest of the target is a trailing gap
    ("AA", "AAAA", 2, -2, 3, 1, 4, "==DD"),
    # ... and the last row before the last column: (4, 2) is the last row's maximum and the last column only equals it
    ("AAAA", "AA", 2, -2, 3, 1, 4, "II=="),
    # row maximum (10, 5) = column maximum (5, 10) = 10: the row wins, the query's prefix and the target's suffix are the end gaps
    ("GGTGGACCAC", "ACCACGGTGG", 2, -2, 3, 1, 10, "IIIII=====DDDDD"),
    # the last column STRICTLY larger (12 against 10): the column wins
    ("GGTGGTACCAC", "ACCACGGTGGT", 2, -2, 3, 1, 12, "DDDDD======IIIII"),
    # H prefers the diagonal over F: either C of the query's CC can stay unpaired; at cell (4, 3) diagonal = F = 3, the diagonal pairs the second C, the first is the gap
    ("AACCGGTTAC", "AACGGTTAC", 2, -2, 3, 1, 15, "==I======="),
    # H prefers the diagonal over E (the mirror)
    ("AACGGTTAC", "AACCGGTTAC", 2, -2, 3, 1, 15, "==D======="),
    # H prefers E over F: at (5, 5) the mismatch costs 5, E = F = 0; E is walked first (backwards), so in alignment order the query-only column comes first
    ("CCCCATTTT", "CCCCGTTTT", 1, -5, 2, 1, 4, "====ID===="),
    # diagonal = E = F (-4 = -2 - 2): the diagonal
    ("CCCCATTTT", "CCCCGTTTT", 1, -4, 2, 1, 4, "====X===="),
    # F prefers extension (open = ext: one run of 2 and two runs of 1 cost the same; rows 4 and 5 form ONE run)
    ("CCAACAAC", "CCAAAC", 2, -2, 2, 2, 8, "===II==="),
    # E prefers extension: AA then ONE run over the target's AC (the other co-optimal path, C against A and a single gap column, opens at the tie)
    ("CAACCA", "AAACCCA", 2, -2, 2, 2, 6, "I==DD==="),
    # a letter outside ACGT scores 0 against itself and is an '=' column; lower against upper case scores as a match and is an 'X' column
    ("ACNT", "ACNT", 2, -2, 3, 1, 6, "===="),
    ("acgt", "ACGT", 2, -2, 3, 1, 8, "XXXX"),
    # empty sequences: n + m gap columns, score 0
    ("", "ACG", 2, -2, 3, 1, 0, "DDD"),
    ("AC", "", 2, -2, 3, 1, 0, "II"),
    # a gap of 2 inside: 20 - (3 + 1)
    ("CCCCCAGTTTTT", "CCCCCTTTTT", 2, -2, 3, 1, 16, "=====II====="),
]


@pytest.mark.parametrize("q,t,ma,mi,op,ex,score,cols", HAND, ids=["%s-%s-%d" % (h[0] or "empty", h[1] or "empty", h[3]) for h in HAND])
def test_reference_reproduces_the_hand_worked_answers(oracle, q, t, ma, mi, op, ex, score, cols):
    r = ref.align_pair(q, t, ma, mi, op, ex)
    assert (r.score, r.cols) == (score, cols)
    sc, cg = oracle.sg_align_cigar_batch(ReadSet.from_strings([q]), ReadSet.from_strings([t]), [0], [0], op, ext=ex, match=ma, mismatch=mi)
    assert (int(sc[0]), cg[0]) == (score, cols)


def test_region_rule_by_hand():
    """one window of all columns when n_cols < k (an empty alignment included), else n_cols - k + 1 windows"""
    assert ref.region("==X==", 2, 2) == 2 and ref.region("==X==", 2, 1) == 4 and ref.region("==X==", 2, 0) == 4 and ref.region("==X==", 2, 3) == 0
    assert ref.region("==X==", 5) == 0 and ref.region("==X==", 5, 4) == 1 and ref.region("==X==", 64, 4) == 1 and ref.region("==X==", 64, 5) == 0
    assert ref.region("", 13, 0) == 1 and ref.region("", 13, -1) == 1 and ref.region("", 13, 1) == 0 and ref.region("", 1) == 0
    assert ref.region("IIDD", 3, 0) == 2 and ref.region("=", 1) == 1 and ref.region("=D=", 1) == 2


def _oracle_case(oracle, case):
    Q = ReadSet.from_strings(list(case.queries)); T = ReadSet.from_strings(list(case.targets))
    kw = dict(ext=case.ext, match=case.match, mismatch=case.mismatch)
    four = oracle.sg_align_batch(Q, T, case.q_idx, case.t_idx, case.open, k=case.k, match_id=None if case.mid_absent else case.match_id, **kw)
    sc, cols = oracle.sg_align_cigar_batch(Q, T, case.q_idx, case.t_idx, case.open, **kw)
    return four, sc, cols


def _describe(case, p, r):
    q, t = case.queries[case.q_idx[p]], case.targets[case.t_idx[p]]
    return "%s pair %d (%s), n %d, m %d, open %d, scheme %d/%d/ext %d, k %d, match_id %d, reference score %d" % (
        case.name, p, case.tags[p] if isinstance(case.tags[p], str) else case.tags[p]["what"], len(q), len(t), case.open[p], case.match, case.mismatch, case.ext, case.k, case.match_id[p], r[0][p])


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_equals_reference(oracle, family):
    for case in ac.cases(family):
        r = ref.case_results(case)
        four, sc, cols = _oracle_case(oracle, case)
        at = np.nonzero(case.ref)[0]
        for nm, a, b in zip(("score", "n_cols", "n_match", "region", "score of the cigar call"), four + (sc,), r[:4] + (r[0],)):
            bad = at[a[at] != b[at]]
            assert len(bad) == 0, "%s: oracle %d, reference %d - %s" % (nm, a[bad[0]], b[bad[0]], _describe(case, int(bad[0]), r))
        for p in at:
            assert cols[p] == r[4][p], "columns - %s\n  oracle    %s\n  reference %s" % (_describe(case, int(p), r), cols[p], r[4][p])


@pytest.mark.parametrize("bit", [1, 2, 4, 8])
def test_family_c_sees_every_tie_break_rule(oracle, bit):
    """the oracle switched to another order of one rule (H: diag > F > E; E / F prefer opening; end cell = last maximum; H prefers a gap) must DIFFER from the
    reference on at least one pair of family c: the family would catch a kernel that took that order"""
    f = oracle.lib.ongsid_debug_sg_tiebreak; f.restype = C.c_int32
    differ = 0
    try:
        f(C.c_int32(bit))
        for case in ac.cases("c"):
            r = ref.case_results(case)
            four, sc, cols = _oracle_case(oracle, case)
            assert np.array_equal(sc, r[0]), "the score does not depend on a tie-break (%s)" % case.name
            differ += sum(1 for p in range(len(cols)) if cols[p] != r[4][p])
    finally:
        f(C.c_int32(0))
    assert differ > 0, "no pair of family c tells tie-break mode %d from the build's rules" % bit
    four, sc, cols = _oracle_case(oracle, ac.cases("c")[0])
    assert list(cols) == list(ref.case_results(ac.cases("c")[0])[4]), "mode 0 was not restored"


# ---- the conditions of the families
def test_cells_checked_against_the_reference_stay_under_the_cap():
    total, per = ac.reference_cells()
    assert total <= CELL_CAP, per
    assert total >= 100_000_000, "the families shrank: %s" % per


def test_family_a_covers_every_instance_boundary_in_both_roles():
    cs = {c.name: c for c in ac.cases("a")}
    for L in ac.A_LENGTHS:
        c = cs["a_L%d" % L]; s = cs["a_L%d_swapped" % L]
        ql = np.array([len(q) for q in c.queries])[c.q_idx]; tl = np.array([len(t) for t in c.targets])[c.t_idx]
        assert ql.max() == L and 20 <= len(c.q_idx) <= 40, (L, ql.max(), len(c.q_idx))
        if L > 7: assert {1, 7, L // 2, L - 1, L} <= set(ql.tolist()), (L, sorted(set(ql.tolist())))
        full = tl[ql == L]
        assert full.min() <= 64
        if L > 1024: assert tl[ql > 400].max() <= 400
        elif L > 2: assert any(abs(x - L) <= 0.12 * L for x in full) and any(x >= 1.7 * L for x in full), (L, full)
        # every pair with the roles swapped: in the call itself while the swapped query fits, and all of them in the swapped call
        have = {(x.queries[a], x.targets[b]) for x in (s, c) for a, b in zip(x.q_idx, x.t_idx)}
        assert all((c.targets[b], c.queries[a]) in have for a, b in zip(c.q_idx, c.t_idx))
        assert len(s.q_idx) >= 10 and all((c.targets[b], c.queries[a]) in {(s.queries[x], s.targets[y]) for x, y in zip(s.q_idx, s.t_idx)} for a, b, t in zip(c.q_idx, c.t_idx, c.tags) if not t.endswith("swapped"))
    # the instances: every class of the int16 kernels, every int32 instance, one to four strips
    longest = [c.meta["L"] for c in ac.cases("a")]
    for lo, hi in zip((0,) + tuple(b for b, _ in ac.RPL32[:-1]), tuple(b for b, _ in ac.RPL32[:-1]) + (4000,)):
        assert any(lo < x <= hi for x in longest) and hi in longest and (hi + 1 in longest or hi == 4000), (lo, hi)
    assert {1, 2, 3, 4} <= {(x + 1023) // 1024 for x in longest}


def _runs(cols):
    """[(kind, first query position, first target position, length)]: maximal runs of 'I', 'D' and of '=' / 'X' together ('M')"""
    out = []; i = j = 0; x = 0
    while x < len(cols):
        kind = "M" if cols[x] in "=X" else cols[x]
        y = x
        while y < len(cols) and ("M" if cols[y] in "=X" else cols[y]) == kind: y += 1
        out.append((kind, i, j, y - x))
        if kind != "D": i += y - x
        if kind != "I": j += y - x
        x = y
    return out


def test_family_b_runs_lie_where_the_cases_say():
    seen_r = set(); gaps = {"I": set(), "D": set(), "M": set()}
    for case in ac.cases("b"):
        r = ref.case_results(case)
        rs_ = case.meta["rows_per_lane"]; seen_r |= set(rs_)
        ql = max(len(q) for q in case.queries)
        assert ql == case.meta["L"] and ac.CLASSES[ac.class_of(ql)][1] in rs_ and [x for b, x in ac.RPL32 if ql <= b][0] in rs_
        for p, tag in enumerate(case.tags):
            if isinstance(tag, str): continue
            runs = _runs(r[4][p])
            for want in tag["runs"]:
                assert tuple(want) in runs, (case.name, tag["what"], want, runs)
                gaps[want[0]].add(want[3])
            interior = [x for x in runs[1:-1] if x[0] != "M"]
            assert len(interior) == len([w for w in tag["runs"] if w[0] != "M"]), (case.name, tag["what"], runs)
            if "boundary" in tag:                      # the vertical run holds the boundary row (1-based B = 0-based B - 1) and, from 2 rows on, the row after it
                _, i0, _, g = tag["runs"][0]; B = tag["boundary"]
                assert i0 <= B - 1 < i0 + g and (g == 1 or i0 <= B < i0 + g), tag
                assert any(B % (r_ * k) == 0 for r_ in rs_ for k in (1, ac.WALK_LANES, 64))
    assert seen_r == {4, 8, 12, 13, 14, 16}
    assert {1, 2} <= gaps["I"] and all({r_ + 1, 8 * r_ + 1} <= gaps["I"] for r_ in seen_r)
    assert gaps["D"] >= {1, 63, 64, 65, 200} and gaps["M"] >= {63, 64, 65, 127, 128, 129}
    strips = [t["boundary"] for c in ac.cases("b") for t in c.tags if not isinstance(t, str) and "boundary" in t and t["boundary"] % 1024 == 0]
    assert {1024, 2048} <= set(strips)


def test_family_c_is_made_of_ties():
    """on the reference alone: every call meets ties (and most of its pairs do), and the family shows each kind"""
    kinds = set()
    for case in ac.cases("c"):
        res = ref.case_results(case)[6]
        tied = sum(1 for x in res if x.tie_cells > 0)
        assert tied >= 0.75 * len(res), (case.name, tied, len(res))
        for x in res: kinds |= x.ties
    assert kinds >= {ref.DIAG_E, ref.DIAG_F, ref.E_F, ref.EXT_OPEN_E, ref.EXT_OPEN_F, ref.ROW_COL, ref.ROW_MULTI, ref.COL_MULTI}, kinds
    c0 = ac.cases("c")[0]; r0 = ref.case_results(c0)
    tags = {t: p for p, t in enumerate(c0.tags)}
    assert ref.ROW_MULTI in r0[6][tags["best score three times in the last row"]].ties and ref.COL_MULTI in r0[6][tags["best score three times in the last column"]].ties
    assert ref.ROW_COL in r0[6][tags["best score once in the last row and once in the last column"]].ties
    p = tags["all N, n < m"]; assert r0[0][p] == 0 and r0[4][p] == "I" * 19 + "=" + "D" * 29      # every cell 0: the first maximum of the last row is column 1
    p = tags["N block against N block"]; assert r0[0][p] == 48 and r0[2][p] == 32 and r0[4][p] == "=" * 32      # N against N: score 0, '=' columns
    p = tags["lower against upper"]; assert r0[0][p] == 24 and r0[2][p] == 0 and r0[4][p] == "X" * 12
    schemes = {(c.ext, int(c.open[0])) for c in ac.cases("c")}
    assert any(e == o for e, o in schemes) and any(o < e for e, o in schemes) and any(e == 0 for e, o in schemes)


def test_family_d_reaches_every_window_case():
    for case in ac.cases("d"):
        r = ref.case_results(case); k = case.k
        ncols = set(r[1].tolist())
        assert {k - 1, k, k + 1} <= ncols, (case.name, sorted(ncols))
        if case.mid_absent: assert (case.match_id == k).all()
        else: assert {-1, 0, 1, k - 1, k, k + 1} == set(case.match_id.tolist())
        p = [x for x, t in enumerate(case.tags) if t.startswith("30 inside 300")][0]
        runs = _runs(r[4][p]); assert runs[0][0] == "D" and runs[-1][0] == "D" and runs[0][3] > k and runs[-1][3] > k, runs
        for p, t in enumerate(case.tags):
            if t.startswith(("empty", "both empty")):
                q, tt = case.queries[case.q_idx[p]], case.targets[case.t_idx[p]]
                assert r[0][p] == 0 and r[1][p] == len(q) + len(tt) and r[2][p] == 0 and r[3][p] == (max(1, r[1][p] - k + 1) if case.match_id[p] <= 0 else 0)
        lens = {len(case.queries[a]) + len(case.targets[b]) for a, b, t in zip(case.q_idx, case.t_idx, case.tags) if t.startswith("empty")}
        assert any(x <= k for x in lens) and any(x > k for x in lens)
        assert len(set(r[3].tolist())) >= 3                                                           # the statistic moves with match_id
    assert {c.k for c in ac.cases("d")} == {1, 2, 13, 63, 64}


def test_family_e_sits_on_both_sides_of_every_bound():
    seen = set()
    for case in ac.cases("e"):
        r = ref.case_results(case)
        ql = max(len(q) for q in case.queries); tl = max(len(t) for t in case.targets)
        app = ac.align16_applicable(case.match, case.mismatch, case.ext, int(case.open.max()), ql, tl)
        assert app == case.meta["applicable"], case.name
        seen.add(case.name)
        if case.name == "e_corner":
            assert (ql, tl) == (896, 4000) and (case.match, case.mismatch, case.ext, int(case.open.max())) == (4, -8, 4, 16)
            assert ac.flag_span(4, 4, 16, 896, 4000, False) < 32768 <= ac.flag_span(4, 4, 16, 896, 4000, True)         # the plain frame holds the corner, the skewed one does not
            assert r[0][0] == 4 * 896 and r[4][0] == "D" * 3104 + "=" * 896 and r[0][1] < 400 < r[0][2] < 4 * 448
        elif not app and ql <= 4000 and tl <= 4000 and "score_above" not in case.meta:
            # one step outside ONE bound: the corner scheme passes when that one value is put back
            vals = [case.match, case.mismatch, case.ext, int(case.open.max())]; corner = [4, -8, 4, 16]
            assert sum(1 for a, b in zip(vals, corner) if a != b) == 1 and all(abs(a - b) <= 1 or b == -8 and a == 1 for a, b in zip(vals, corner))
        if "score_above" in case.meta: assert r[0].max() > 32767 and r[0].max() == 9 * 4000
    assert {"e_corner", "e_open17", "e_ext5", "e_match5", "e_mismatch-9", "e_mismatch+1", "e_m4001", "e_n4001", "e_score_above_int16"} == seen
    assert max(len(t) for t in [c for c in ac.cases("e") if c.name == "e_m4001"][0].targets) == 4001
    assert max(len(q) for q in [c for c in ac.cases("e") if c.name == "e_n4001"][0].queries) == 4001


def test_family_f_fills_every_bin_of_the_paired_kernel():
    (case,) = ac.cases("f")
    n = len(case.q_idx)
    assert ac.PARTITION_MIN_PAIRS < n <= ac.PARTITION_MIN_PAIRS + 16
    ql = np.array([len(q) for q in case.queries])[case.q_idx]; tl = np.array([len(t) for t in case.targets])[case.t_idx]
    assert ql.max() > ac.CLASSES[0][0] and ql.max() <= 896 and ql[:4095].max() > ac.CLASSES[0][0]
    assert (tl == 4001).sum() == 3 and tl[tl != 4001].max() <= ac.ALIGN16_MAXLEN
    short = tl <= ac.ALIGN16_MAXLEN                                                               # (the others are the int32 class)
    for c, (bound, _, R) in enumerate(ac.CLASSES[:4]):
        lo = 0 if c == 0 else ac.CLASSES[c - 1][0]
        odd = 0
        for res in range(R):
            b = short & (ql > lo) & (ql <= bound) & ((ql - 1) % R == res) & (ql > 0)
            assert b.sum() >= 3, (c, res)
            assert tl[b].max() >= 4 * max(1, tl[b].min()), (c, res, tl[b].min(), tl[b].max())
            odd += int(b.sum()) % 2
        assert odd >= 1, "class %d has no bin with an odd count" % c
    edge = case.ref & np.array([not t.startswith(("class", "m = 4 001")) for t in case.tags])
    assert 250 <= edge.sum() <= 320 and {t[0] for t, e in zip(case.tags, edge) if e} == set("abcd")
    wild = np.array([("N" in case.queries[a]) or ("N" in case.targets[b]) or ("n" in case.queries[a]) for a, b in zip(case.q_idx, case.t_idx)])
    assert 0.07 * n <= wild.sum() <= 0.16 * n
    side = case.mismatch + case.open + case.ext
    assert (side < 0).sum() > n // 4 and (side >= 0).sum() > n // 4 and set(case.open.tolist()) == set(ac.F_OPENS)
    fill = np.array([t == "filler" for t in case.tags]); assert (~case.ref[fill]).all() and ql[fill].min() >= 20 and ql[fill].max() <= 60


def test_family_g_indexes_are_not_the_identity():
    (case,) = ac.cases("g")
    assert set(range(len(case.queries))) - set(case.q_idx.tolist()) and set(range(len(case.targets))) - set(case.t_idx.tolist())                # unused reads
    assert "" in [case.queries[a] for a in case.q_idx] and "" in [case.targets[b] for b in case.t_idx]
    assert max(np.bincount(case.q_idx)) >= len(case.targets) - 2                                                                                 # one query against every target
    assert (np.diff(case.t_idx[:8].astype(int)) < 0).all() and case.mid_absent


def test_family_s_strands_are_unambiguous():
    """the strand rule of the polisher (tests/polish_reference.py restates it from the header) calls every read of family s as it was built, with a clear margin"""
    groups = ac.family_s() + [ac.family_s_many()[0]]
    assert [len(g.backbone) for g in groups[:-1]] == list(ac.S_BACKBONES)
    for g in groups:
        fwd = set(pref.minimizers(g.backbone, 13, 20)); rev = set(pref.minimizers(pref.revcomp(g.backbone), 13, 20))
        for x, (read, s) in enumerate(zip(g.reads, g.strand)):
            if g.name == "s_many" and x not in ac.family_s_many()[1]: continue
            a, b, st = pref.strand_call(read, fwd, rev, 13, 20)
            assert st == s and abs(a - b) >= 4 and max(a, b) >= 3 * min(a, b), (g.name, x, a, b, s)
        if g.name != "s_many":
            assert 10 <= sum(1 for s in g.strand if s == 0) <= 20 and sum(g.strand) >= 3 and min(len(r) for r in g.reads) >= 190
    many, checked = ac.family_s_many()
    assert len(many.reads) > ac.PARTITION_MIN_PAIRS and len(set(checked)) == 200 and max(len(r) for r in many.reads) > ac.CLASSES[0][0]
