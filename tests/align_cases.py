"""Deterministic builders of the edge families of the semi-global affine (Gotoh) aligners - k_sg_align, k_sg_align16, k_sg_align16p and their shared
traceback walk: fixed seeds, plain functions, no tests, no GPU.

cases(family) returns a list of Case: one Case is ONE call of sg_align_batch - queries, targets, q_idx, t_idx, a per-pair `open`, (match, mismatch, ext), k, a
per-pair match_id (`mid_absent`: the call passes none, which means k) - plus `tags` (what the builder intended per pair: a string, or a dict the CPU test checks
against the REFERENCE's columns, never assumed), `ref` (per pair: checked against align_reference; the others against the oracle only) and `meta`.  The kernel
instance is chosen per CALL by its longest query (and per pair in a partitioned batch), so a family that aims at several instances is several calls.  The
reference keeps one DP per distinct (query, target, scheme, open): repeated pairs are free.

The constants the builders rely on are restated here and asserted against the sources by test_align_reference_cpu.py:
    CLASSES      kAlignClass of k_align.hip: (longest query, rows per lane of k_sg_align16 = 2 RP, R of the paired kernel or 0)
    RPL32        the int32 instances of ngsid_launch_align: (longest query, rows per lane)
    a lane owns `rows per lane` consecutive rows, 64 lanes make a strip, the traceback walk works in blocks of 64 steps x 8 lanes
"""
from collections import namedtuple
import numpy as np

Case = namedtuple("Case", "name family queries targets q_idx t_idx open match mismatch ext k match_id mid_absent tags ref meta")
ACGT = "ACGT"
CLASSES = ((256, 4, 4), (512, 8, 8), (768, 12, 12), (896, 14, 14), (0xffffffff, 16, 0))
RPL32 = ((256, 4), (512, 8), (768, 12), (832, 13), (896, 14), (0xffffffff, 16))
ALIGN16_MAXLEN = 4000
PARTITION_MIN_PAIRS = 4096
NEG16 = -20000
WALK_STEPS, WALK_LANES = 64, 8
A_LENGTHS = (1, 2, 255, 256, 257, 511, 512, 513, 767, 768, 769, 832, 833, 895, 896, 897, 1023, 1024, 1025, 2048, 2049, 3073, 4000)


def flag_span(match, ext, open_, qlen, tlen, skew):
    """sg16p_flag_span of k_align_common.h"""
    return -NEG16 + ext + open_ + match * min(qlen, tlen) + ((qlen + tlen + 1) * ext if skew else 0)


def align16_applicable(match, mismatch, ext, max_open, max_qlen, max_tlen):
    """ngsid_align16_applicable of k_align.hip"""
    return max_qlen <= ALIGN16_MAXLEN and max_tlen <= ALIGN16_MAXLEN and 0 <= match <= 4 and -8 <= mismatch <= 0 and 0 <= ext <= 4 and 0 <= max_open <= 16


def class_of(n):
    c = 0
    while n > CLASSES[c][0]: c += 1
    return c


def rseq(rng, n, letters=ACGT):
    return "".join(letters[x] for x in rng.integers(0, len(letters), n))


def other(rng, ch):
    return ACGT[(ACGT.index(ch.upper()) + int(rng.integers(1, 4))) % 4] if ch.upper() in ACGT else "A"


def mutate(rng, s, rate):
    """substitutions, deletions and insertions, a third of `rate` each"""
    out = []
    for ch in s:
        u = rng.random()
        if u < rate / 3: continue
        if u < 2 * rate / 3: out.append(ACGT[rng.integers(0, 4)])
        out.append(other(rng, ch) if u > 1 - rate / 3 else ch)
    return "".join(out)


def hp_rich(rng, n):
    out = []
    while sum(map(len, out)) < n: out.append(ACGT[rng.integers(0, 4)] * int(rng.integers(1, 9)))
    return "".join(out)[:n]


def tandem(rng, n, period=None):
    p = int(rng.integers(2, 7)) if period is None else period
    u = rseq(rng, p)
    return (u * (n // p + 1))[:n]


def fit(rng, s, n):
    """s cut or padded (random letters) to exactly n bases"""
    return s[:n] if len(s) >= n else s + rseq(rng, n - len(s))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


class _Build:
    """collects the distinct sequences and the pairs of one call"""
    def __init__(self):
        self.q, self.t, self.qi, self.ti, self.open, self.mid, self.tags, self.ref = [], [], [], [], [], [], [], []
        self._q, self._t = {}, {}

    def qid(self, s):
        if s not in self._q: self._q[s] = len(self.q); self.q.append(s)
        return self._q[s]

    def tid(self, s):
        if s not in self._t: self._t[s] = len(self.t); self.t.append(s)
        return self._t[s]

    def pair(self, q, t, tag, open_=3, mid=None, ref=True):
        self.qi.append(self.qid(q)); self.ti.append(self.tid(t)); self.open.append(open_); self.mid.append(mid); self.tags.append(tag); self.ref.append(ref)

    def both(self, q, t, tag, open_=3, mid=None, swap_below=None):
        """the pair and the pair with the roles swapped (row-before-column in the end cell is asymmetric); the swapped one only while its query stays at
        or below swap_below bases, so that the longest query of the call remains what the case says"""
        self.pair(q, t, tag, open_, mid)
        if swap_below is None or len(t) <= swap_below: self.pair(t, q, tag + " swapped", open_, mid)

    def case(self, name, family, scheme=(2, -2, 1), k=13, mid_absent=False, meta=None):
        mid = np.array([k if x is None else x for x in self.mid], dtype=np.int32)
        if mid_absent: assert all(x is None for x in self.mid)
        return Case(name, family, tuple(self.q), tuple(self.t), np.array(self.qi, dtype=np.uint32), np.array(self.ti, dtype=np.uint32), np.array(self.open, dtype=np.int32),
                    scheme[0], scheme[1], scheme[2], k, mid, mid_absent, tuple(self.tags), np.array(self.ref, dtype=bool), dict(meta or {}))


# ---- a: instance boundaries
def family_a():
    """per longest-query length L one call that holds L plus shorter queries (1, 7, L / 2, L - 1; a short query in a large instance is a case of its own) against targets of
    <= 64, ~ n and ~ 2 n bases (<= 400 above 1 024 rows), mutated / unrelated / homopolymer-rich / tandem content, every pair in both roles while the swapped query fits under
    L; and a second call with ALL pairs swapped (its longest query is the longest target).  107 M cells."""
    out = []
    for L in A_LENGTHS:
        rng = np.random.default_rng(1000 + L)
        pairs = []                                                                                  # (query, target, tag)
        big = L > 1024
        tpl = rseq(rng, 2 * L + 40)                                                                 # the template everything related is cut from
        full = fit(rng, mutate(rng, tpl[L // 2:L // 2 + L], 0.1), L)
        kinds = ("unrelated", "homopolymer", "tandem")
        alt = kinds[A_LENGTHS.index(L) % 3]
        def content(kind, n):
            return rseq(rng, n) if kind == "unrelated" else hp_rich(rng, n) if kind == "homopolymer" else tandem(rng, n)
        if big:
            pairs += [(full, tpl[L // 2 + 100:L // 2 + 130], "L x 30 inside"), (full, mutate(rng, tpl[L - 75:L + 75], 0.1), "L x 150 mutated"),
                      (full, fit(rng, mutate(rng, tpl[L // 2 + L - 200:L // 2 + L + 200], 0.1), 400), "L x 400 across the query's end"),
                      (full, content(alt, 64), "L x 64 " + alt)]
            qh = fit(rng, mutate(rng, tpl[L // 2:L], 0.1), L // 2); q1 = fit(rng, mutate(rng, tpl[L // 2:L // 2 + L], 0.1), L - 1)
            pairs += [(q1, mutate(rng, tpl[L - 75:L + 75], 0.1), "L-1 x 150"), (q1, tpl[L // 2:L // 2 + 40], "L-1 x 40 at the query's start"),
                      (qh, fit(rng, mutate(rng, tpl[L // 2 + 50:L // 2 + 450], 0.1), 400), "L/2 x 400"), (qh, hp_rich(rng, 60), "L/2 x 60 homopolymer")]
        else:
            near = max(1, L - 1 - int(rng.integers(0, 8)))
            pairs += [(full, fit(rng, mutate(rng, tpl[L // 2 + L // 3:L // 2 + L // 3 + 50], 0.1), min(50, max(1, L - 1))), "L x <= 64 inside"),
                      (full, fit(rng, mutate(rng, tpl[L // 2:L // 2 + L], 0.1), near), "L x ~n mutated"),
                      (full, content(alt, max(1, int(0.9 * L))), "L x ~n " + alt),
                      (full, mutate(rng, tpl[:2 * L], 0.1) or "A", "L x ~2n mutated around")]
            if L > 2:
                q1 = fit(rng, mutate(rng, tpl[L // 2:L // 2 + L], 0.1), L - 1); qh = fit(rng, mutate(rng, tpl[L // 2:L], 0.1), L // 2)
                pairs += [(q1, fit(rng, mutate(rng, tpl[L // 2 + L // 3:L // 2 + L], 0.1), max(1, L // 3)), "L-1 x n/3 mutated, up to the query's end"), (q1, content(kinds[(A_LENGTHS.index(L) + 1) % 3], 64), "L-1 x 64 alt"),
                          (qh, fit(rng, mutate(rng, tpl[L // 2:L], 0.1), max(1, L // 2 - 3)), "L/2 x ~n mutated"), (qh, tandem(rng, 40), "L/2 x 40 tandem"),
                          (qh, content(kinds[(A_LENGTHS.index(L) + 2) % 3], 64), "L/2 x 64 alt")]
        q7 = tpl[L // 2 + 3:L // 2 + 10] if L >= 7 else "ACGTTGA"[:max(L, 1)]
        pairs += [(q7, tpl[L // 2:L // 2 + 14], "7 x 14 inside"), (q7, fit(rng, mutate(rng, q7, 0.2), 7), "7 x 7"), (q7, hp_rich(rng, 64), "7 x 64 homopolymer"),
                  (q7, fit(rng, tpl[max(0, L // 2 - 90):L // 2 + 110], 200), "7 x 200 inside"),
                  (tpl[L // 2], tpl[L // 2], "1 x 1"), (tpl[L // 2], rseq(rng, 3), "1 x 3"), (tpl[L // 2], tpl[max(0, L // 2 - 20):L // 2 + 20], "1 x <= 40")]
        if L <= 2: pairs += [(rseq(rng, L), rseq(rng, 1 + 7 * x), "L x %d" % (1 + 7 * x)) for x in range(10)]
        pairs = [(q[:L], t, tag) for q, t, tag in pairs]                                           # (L = 1, 2: the short queries are cut to the instance's length)
        b = _Build(); s = _Build()
        for x, (q, t, tag) in enumerate(pairs):
            b.both(q, t, tag, open_=2 + x % 4, mid=9, swap_below=L)
            s.pair(t, q, tag + " swapped", open_=2 + x % 4, mid=9)
        assert max(len(q) for q in b.q) == L
        out.append(b.case("a_L%d" % L, "a", meta={"L": L}))
        out.append(s.case("a_L%d_swapped" % L, "a", meta={"L": max(len(q) for q in s.q)}))
    return out


# ---- b: paths that cross structure
def _no_slide(rng, n, before, after):
    """n random bases whose first differs from `after` and whose last differs from `before`: the gap that removes them cannot slide over an equal neighbour"""
    while True:
        s = rseq(rng, n)
        if s[-1] != before and s[0] != after: return s


def family_b():
    """query = X + INS + Y against target = X + Y (a vertical gap: 'I' columns over rows |X| + 1 ... |X| + g) and the mirror (a horizontal gap: 'D' columns), one call per
    instance (rows per lane r = 4, 8, 12, 13 and 14, 14, 16).  Vertical gaps of 1, 2, r + 1 and 8 r + 1 rows straddle a lane's last row, the last row of a group of 8 lanes
    and (r = 16) the last rows of strips 1 and 2; horizontal gaps of 1, 63, 64, 65 and 200 columns sit in a lane's last row and in the first row of a group; diagonal runs of
    exactly 63 ... 129 columns lie between an 'I' and a 'D' run.  tags: {"runs": [(op, first query position, first target position, length), ...]} - asserted on the
    reference's columns.  30 M cells, most of them in the strip-boundary pairs."""
    out = []
    for Lcall, rs_ in ((256, (4,)), (512, (8,)), (768, (12,)), (832, (13, 14)), (896, (14,)), (2304, (16,))):
        rng = np.random.default_rng(2000 + Lcall)
        b = _Build()
        def vertical(B, g, why):
            nx = B - 1 if g == 1 else B - g // 2
            ny = g // 2 + 40                                                                  # (enough matches after the gap that ending the alignment before it is worse)
            if nx < g // 2 + 20 or nx + g + ny > Lcall: return False
            X, Y = rseq(rng, nx), rseq(rng, ny)
            ins = _no_slide(rng, g, X[-1], Y[0])
            b.pair(X + ins + Y, X + Y, {"what": "vertical gap of %d rows over %s (row %d)" % (g, why, B), "runs": [("I", nx, nx, g)], "boundary": B})
            return True
        def horizontal(rows, g, why):
            row = [x for x in rows if x >= g // 2 + 12][0]                                        # (enough matches before the gap that starting the alignment after it is worse)
            X, Y = rseq(rng, row), rseq(rng, g // 2 + 20)
            assert len(X) + len(Y) <= Lcall
            ins = _no_slide(rng, g, X[-1], Y[0])
            b.pair(X + Y, X + ins + Y, {"what": "horizontal gap of %d columns in %s (row %d)" % (g, why, row), "runs": [("D", row, row, g)]})
        for r in rs_:
            for g in (1, 2, r + 1, 8 * r + 1):
                assert vertical(3 * r, g, "a lane's last row, r = %d" % r) or vertical(27 * r, g, "a lane's last row, r = %d" % r)
                assert vertical(8 * r, g, "a group's last row, r = %d" % r) or vertical(16 * r, g, "a group's last row, r = %d" % r)
                if Lcall > 1024:
                    assert vertical(64 * r, g, "strip 1's last row") and vertical(128 * r, g, "strip 2's last row")
            for g in (1, 63, 64, 65, 200):
                horizontal([r * l for l in range(3, 64) if l % 8], g, "a lane's last row, r = %d" % r); horizontal([8 * r * l + 1 for l in range(1, 8)], g, "a group's first row, r = %d" % r)
            for d in (63, 64, 65, 127, 128, 129):
                nx = 5 * r - 2                                                                    # the 'I' run covers rows 5 r - 1, 5 r: the diagonal run starts on a lane's first row
                X, M, Y = rseq(rng, nx), rseq(rng, d), rseq(rng, 40)
                i1 = _no_slide(rng, 2, X[-1], M[0]); d1 = _no_slide(rng, 3, M[-1], Y[0])
                b.pair(X + i1 + M + Y, X + M + d1 + Y, {"what": "diagonal run of %d between two gaps, r = %d" % (d, r), "runs": [("I", nx, nx, 2), ("M", nx + 2, nx, d), ("D", nx + 2 + d, nx + d, 3)]})
        q = rseq(rng, Lcall)
        b.pair(q, q[Lcall // 2:Lcall // 2 + 48], "the query that selects the instance")
        out.append(b.case("b_L%d" % Lcall, "b", meta={"L": Lcall, "rows_per_lane": rs_}))
    return out


# ---- c: ties
C_SCHEMES = {"2/-2/1/3": (2, -2, 1, 3), "open=ext": (2, -2, 2, 2), "open<ext": (2, -2, 3, 1), "ext=0": (2, -2, 0, 3), "1/-3/2/2": (1, -3, 2, 2), "1/-5/1/2": (1, -5, 1, 2)}


def family_c():
    """inputs made of ties: homopolymers of unequal length, tandem repeats with one unit removed or added, all-N pairs and N blocks (score 0, '=' columns), lower against
    upper case (scores as a match, 'X' columns), and pairs whose best score occurs several times in the last row, in the last column, and once in each - under 2/-2/1/3,
    open = ext, open < ext, ext = 0 and a mismatch dearer than two gaps (E = F without the diagonal).  One call per scheme.  Small (< 2 M cells)."""
    rng = np.random.default_rng(3000)
    pairs = []
    for n, m in ((5, 9), (9, 9), (9, 5), (64, 70), (64, 64), (70, 64), (200, 130), (1, 4), (4, 1)):
        pairs.append(("A" * n, "A" * m, "A x %d against A x %d" % (n, m)))
    for p in range(1, 7):
        u = rseq(rng, p) if p > 1 else "C"
        while p > 1 and len(set(u)) == 1: u = rseq(rng, p)
        for reps in (6, 41):
            pairs.append((u * (reps - 1), u * reps, "period %d, %d units, one removed" % (p, reps)))
            pairs.append((u * (reps + 1), u * reps, "period %d, %d units, one added" % (p, reps)))
        pairs.append((u.lower() * 9, u * 8, "period %d lower against upper, one added" % p))
    fl, fr = rseq(rng, 12), rseq(rng, 12)
    pairs += [("N" * 20, "N" * 30, "all N, n < m"), ("N" * 30, "N" * 20, "all N, n > m"), ("N" * 7, "N" * 7, "all N, n = m"),
              (fl + "N" * 8 + fr, fl + "N" * 8 + fr, "N block against N block"), (fl + "N" * 8 + fr, fl + "N" * 5 + fr, "N block against a shorter N block"),
              (fl + "NNNN" + fr, fl + "ACGT" + fr, "N block against letters"), ("n" * 6 + fl, "N" * 6 + fl, "n against N"),
              ("acgtacgtacgt", "ACGTACGTACGT", "lower against upper"), ("acgtacgtacgt", "ACGTACGTACGTACGT", "lower against upper, one unit more"),
              ((fl + fr).lower(), fl + "G" + fr, "lower against upper with a gap")]
    w = "ACGTTGCA"
    pairs += [(w, "TT".join([w] * 3), "best score three times in the last row"), ("TT".join([w] * 3), w, "best score three times in the last column"),
              ("GGTGG" + "ACCAC", "ACCAC" + "GGTGG", "best score once in the last row and once in the last column"),
              ("GGTGGT" + "ACCAC", "ACCAC" + "GGTGGT", "the last column strictly better than the last row"),
              ("ACGT" + "TTTTT" + "GACC", "ACGT" + "GACC", "an insertion inside a homopolymer flank"), ("ACGTT" + "GACC", "ACGTT" + "TTTT" + "TGACC", "a deletion that can slide"),
              ("ACGTACCGTA", "ACGTCAGTA", "a substitution or two gaps"), ("AACCGGTT", "AACGGTT", "one base of a run removed"), ("AACGGTT", "AACCGGTT", "one base of a run added"),
              ("CCCCATTTT", "CCCCGTTTT", "a substitution, or a gap on either side first"), (fl + "A" + fr, fl + "G" + fr, "a substitution between flanks"),
              ("CCAACAAC", "CCAAAC", "one gap of two or two gaps of one (F)"), ("CAACCA", "AAACCCA", "one gap of two or a mismatch and a gap (E)"),
              ("AACCAAC", "CCCAAAC", "extension or opening (E), after an end gap"), ("CACCCAAA", "CACCAAC", "extension or opening (F), before an end gap")]
    out = []
    for name, (ma, mi, ext, op) in C_SCHEMES.items():
        b = _Build()
        for q, t, tag in pairs: b.pair(q, t, tag, open_=op, mid=7)
        out.append(b.case("c_" + name, "c", scheme=(ma, mi, ext), k=13, meta={"scheme": name}))
    return out


# ---- d: the window statistic
D_KS = (1, 2, 13, 63, 64)


def family_d():
    """k in 1, 2, 13, 63, 64 x match_id in -1, 0, 1, k - 1, k, k + 1 (one call per k) and absent (a second call per k), over alignments of k - 1, k and k + 1 columns, a
    30-base query inside a 300-base target (both end-gap runs exceed k), empty queries and targets with n + m <= k and > k, and two ordinary pairs.  Small."""
    out = []
    for k in D_KS:
        rng = np.random.default_rng(4000 + k)
        t300 = rseq(rng, 300); base = rseq(rng, 100)
        pairs = []
        for n in (k - 1, k, k + 1):
            s = rseq(rng, n)
            pairs.append((s, s, "identical, %d columns (k %+d)" % (n, n - k)))
            if n >= 3: pairs.append((s, s[:n // 2] + other(rng, s[n // 2]) + s[n // 2 + 1:], "one substitution, %d columns" % n))
        pairs += [(t300[140:170], t300, "30 inside 300"), (t300, t300[140:170], "300 around 30"),
                  ("", rseq(rng, max(k - 1, 1)), "empty query, m <= k"), ("", rseq(rng, k + 5), "empty query, m > k"), (rseq(rng, max(k - 1, 1)), "", "empty target, n <= k"),
                  (rseq(rng, k + 5), "", "empty target, n > k"), ("", "", "both empty"),
                  (mutate(rng, base, 0.15), base, "mutated 100"), (base[:60].lower() + base[60:], base, "60 lower-case bases: 'X' columns that score as matches"),
                  ("N" * 20 + base[20:], "N" * 20 + base[20:], "20 N against N: '=' columns that score 0")]
        b = _Build(); a = _Build()
        for q, t, tag in pairs:
            for mid in (-1, 0, 1, k - 1, k, k + 1): b.pair(q, t, tag + ", match_id %d" % mid, mid=mid)
            a.pair(q, t, tag + ", match_id absent")
        out.append(b.case("d_k%d" % k, "d", k=k)); out.append(a.case("d_k%d_absent" % k, "d", k=k, mid_absent=True))
    return out


# ---- e: range corners
def family_e():
    """the corner of ngsid_align16_applicable (4/-8/ext 4/open 16, n = 896, m = 4 000: identical at the target's end, unrelated, half matching), one step outside each of its
    bounds (open 17, ext 5, match 5, mismatch -9, mismatch +1, m = 4 001, n = 4 001: the int32 kernel, the same answers) and one score above 32 767 (match 9 on identical
    4 000-base sequences).  meta: applicable (the int16 kernels take the call), score_above.  32 M cells."""
    rng = np.random.default_rng(5000)
    out = []
    t4k = rseq(rng, 4000)
    b = _Build()
    b.pair(t4k[-896:], t4k, "identical at the target's end", open_=16)
    b.pair(rseq(rng, 896), t4k, "unrelated", open_=16)
    b.pair(t4k[1500:1948] + rseq(rng, 448), t4k, "half matching", open_=16)
    b.pair(mutate(rng, t4k[2000:2300], 0.1), t4k[1900:2400], "300 mutated inside 500", open_=16)
    out.append(b.case("e_corner", "e", scheme=(4, -8, 4), meta={"applicable": True}))
    base = rseq(rng, 320)
    small = [(fit(rng, mutate(rng, base, 0.12), 300), base, "300 mutated"), (rseq(rng, 280), base, "unrelated"), (hp_rich(rng, 260), hp_rich(rng, 300), "homopolymer-rich"),
             (base[40:300], base, "identical inside"), (base, base[40:300], "identical around"), (tandem(rng, 257, 3), tandem(rng, 270, 3), "tandem")]
    for name, (ma, mi, ext, op) in (("open17", (4, -8, 4, 17)), ("ext5", (4, -8, 5, 16)), ("match5", (5, -8, 4, 16)), ("mismatch-9", (4, -9, 4, 16)), ("mismatch+1", (4, 1, 4, 16))):
        b = _Build()
        for q, t, tag in small: b.pair(q, t, tag, open_=op)
        out.append(b.case("e_" + name, "e", scheme=(ma, mi, ext), meta={"applicable": False}))
    t4001 = t4k + "G"
    b = _Build()
    b.pair(mutate(rng, t4001[3700:], 0.1), t4001, "~300 mutated at the end of 4 001", open_=16); b.pair(rseq(rng, 257), t4001, "unrelated x 4 001", open_=16)
    out.append(b.case("e_m4001", "e", scheme=(4, -8, 4), meta={"applicable": False}))
    b = _Build()
    b.pair(t4001, mutate(rng, t4001[2000:2060], 0.1), "4 001 x ~60 mutated", open_=16); b.pair(t4001, t4001[-40:], "4 001 x 40 at the end", open_=16)
    out.append(b.case("e_n4001", "e", scheme=(4, -8, 4), meta={"applicable": False}))
    b = _Build()
    b.pair(t4k, t4k, "identical 4 000 under match 9", open_=16)
    out.append(b.case("e_score_above_int16", "e", scheme=(9, -8, 4), meta={"applicable": False, "score_above": 32767}))
    return out


# ---- f: the partitioned batch and the paired kernel
F_SCHEME = (4, -8, 1)
F_OPENS = (4, 5, 6, 7, 8, 9)          # mismatch + open + ext >= 0 from open 7 on


def family_f():
    """ONE call of 4 096 + a few pairs under 4/-8/ext 1 with per-pair opens 4 ... 9: ~ 300 edge pairs of families a - d with n <= 896 (small ones: n x m <= 60 000), for
    every (class, residue (n - 1) mod R) bin of the paired kernel at least three pairs whose targets differ wildly in length - one with a 40-base target (reference), the others
    ~ n and ~ 2 n (oracle only) -, three pairs with m = 4 001 (the int32 class of a partitioned batch), and fillers of 20 - 60 bases (oracle only); every tenth filler and
    every tenth bin pair carries a wildcard.  The first 4 095 pairs of the same list take the single-launch route.  The order is shuffled, so the launcher's pairing inside a
    bin meets both kinds of neighbour.  5 M reference cells."""
    rng = np.random.default_rng(6000)
    items = []                                                                                    # (q, t, tag, ref)
    seen = set()
    for fam in "abcd":
        for case in cases(fam):
            for p in range(len(case.q_idx)):
                q, t = case.queries[case.q_idx[p]], case.targets[case.t_idx[p]]
                if len(q) <= 896 and len(q) * len(t) <= 60000 and (q, t) not in seen and len(q) > 0:
                    seen.add((q, t)); items.append((q, t, "%s pair %d: %s" % (case.name, p, case.tags[p] if isinstance(case.tags[p], str) else case.tags[p]["what"]), True))
    items = [items[x] for x in np.unique(np.linspace(0, len(items) - 1, 300).astype(int))]
    tpl = rseq(rng, 2000)
    x = 0
    for c, (bound, _, R) in enumerate(CLASSES[:4]):
        lo = 1 if c == 0 else CLASSES[c - 1][0] + 1
        for res in range(R):
            ns = [n for n in range(lo, bound + 1) if (n - 1) % R == res]
            count = 3 + (1 if (res % 2 and res > 0) else 0)                                        # residue 0 keeps an odd count (edge pairs and fillers only ever ADD to class 0's bins: asserted, not assumed)
            for v in range(count):
                n = ns[int(rng.integers(0, len(ns)))] if c else ns[-1 - v] if len(ns) > v else ns[-1]
                a = int(rng.integers(0, 600))
                q = fit(rng, mutate(rng, tpl[a:a + n], 0.1), n)
                if x % 10 == 0: q = q[:n // 2] + "N" + q[n // 2 + 1:]
                if v == 0: items.append((q, tpl[a + n // 3:a + n // 3 + 40], "class %d residue %d, 40-base target" % (c, res), True))
                elif v == 1: items.append((q, mutate(rng, tpl[a:a + n], 0.1) or "A", "class %d residue %d, target ~ n" % (c, res), False))
                else: items.append((q, tpl[max(0, a - n // 2):a + n + n // 2], "class %d residue %d, target ~ 2 n" % (c, res), False))
                x += 1
    t4001 = rseq(rng, 4001)
    for v in range(3): items.append((mutate(rng, t4001[1000 * v + 100:1000 * v + 130], 0.1), t4001, "m = 4 001 (the int32 class)", True))
    ft = [rseq(rng, int(rng.integers(20, 61))) for _ in range(40)]
    while len(items) < PARTITION_MIN_PAIRS + 7:
        t = ft[int(rng.integers(0, len(ft)))]
        q = mutate(rng, t, 0.15) if rng.random() < 0.8 else rseq(rng, int(rng.integers(20, 61)))
        q = fit(rng, q, max(20, min(60, len(q))))
        if len(items) % 10 == 0: q = q[:5] + "N" + q[6:]
        items.append((q, t, "filler", False))
    order = rng.permutation(len(items))
    b = _Build()
    for x, o in enumerate(order):
        q, t, tag, r = items[o]
        b.pair(q, t, tag, open_=F_OPENS[x % len(F_OPENS)], mid=9, ref=r)
    return [b.case("f_partitioned", "f", scheme=F_SCHEME, k=13)]


# ---- g: indexing and call hygiene
def family_g():
    """non-identity q_idx / t_idx: one query against many targets, the pairs in reversed order, unused and empty reads in both sets.  Small."""
    rng = np.random.default_rng(7000)
    base = rseq(rng, 300)
    targets = [mutate(rng, base[a:a + n], 0.1) for a, n in ((0, 300), (50, 120), (100, 40), (0, 64), (200, 100), (10, 257), (150, 7))] + ["", rseq(rng, 90), "N" * 12, base.lower()[:80]]
    queries = ["", mutate(rng, base[20:280], 0.08), rseq(rng, 33), mutate(rng, base[100:160], 0.1), "", base[30:31], hp_rich(rng, 70)]
    b = _Build()
    b.q = [rseq(rng, 50)] + queries + [rseq(rng, 400)]; b.t = [rseq(rng, 500)] + targets + [rseq(rng, 10)]      # the first and the last read of either set stay unused
    def add(qi, ti, tag): b.qi.append(qi); b.ti.append(ti); b.open.append(2 + (qi + ti) % 4); b.mid.append(None); b.tags.append(tag); b.ref.append(True)
    for ti in range(len(targets), 0, -1): add(2, ti, "one query against every target, last target first")
    for qi in range(len(queries), 0, -1):
        for ti in (1, 3, 8): add(qi, ti, "queries in reversed order")
    for ti in (8, 8, 2, 2): add(1, ti, "an empty query, repeated")
    out = [b.case("g_indexing", "g", k=13, mid_absent=True)]
    return out


# ---- s: spans of the polisher's affine read -> backbone alignment (aln_mode 0)
SGroup = namedtuple("SGroup", "name backbone reads strand")
S_BACKBONES = (499, 500, 501, 1000, 1001, 1050)
S_SCORES = dict(aln_match=2, aln_mismatch=-2, aln_open=3, aln_ext=1)


def _family_s():
    """per backbone length (the polishing window is 500: one window, the 10 % tail rule, two and three windows) 15 plus-strand reads of 200 - 330 bases cut from the
    backbone at starts that put window boundaries inside them, 5 % errors, every fifth reverse-complemented.  strand: what the builder made (asserted with the strand rule).
    21 M cells."""
    out = []
    for B in S_BACKBONES:
        rng = np.random.default_rng(8000 + B)
        bb = rseq(rng, B)
        reads, strand = [], []
        for x in range(18):
            n = int(rng.integers(200, 331)); a = int(x * (B - n) / 17)
            r = mutate(rng, bb[a:a + n], 0.05)
            if x % 5 == 4: r = revcomp(r)
            reads.append(r); strand.append(1 if x % 5 == 4 else 0)
        out.append(SGroup("s_B%d" % B, bb, tuple(reads), tuple(strand)))
    return out


def _family_s_many():
    """one group of 4 300 reads against a 501-base backbone: reads of 110 - 170 bases and every fiftieth of 260 - 300 (the call is partitioned only when a query exceeds 256
    bases), 4 % errors, every seventh reverse-complemented; `checked`: the 200 reads compared with the reference.  17 M cells."""
    rng = np.random.default_rng(8999)
    bb = rseq(rng, 501)
    reads, strand = [], []
    for x in range(4300):
        n = int(rng.integers(260, 301)) if x % 50 == 0 else int(rng.integers(110, 171)); a = int(rng.integers(0, 501 - n + 1))
        r = mutate(rng, bb[a:a + n], 0.04)
        if x % 7 == 3: r = revcomp(r)
        reads.append(r); strand.append(1 if x % 7 == 3 else 0)
    checked = tuple(range(0, 4300, 50))[:40] + tuple(x for x in range(1, 4300, 21) if x % 50)[:160]
    return SGroup("s_many", bb, tuple(reads), tuple(strand)), checked


def family_s():
    if "s" not in _built: _built["s"] = _family_s()
    return _built["s"]


def family_s_many():
    if "s_many" not in _built: _built["s_many"] = _family_s_many()
    return _built["s_many"]


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e, "f": family_f, "g": family_g}
_built = {}


def cases(family):
    if family not in _built: _built[family] = FAMILIES[family]()
    return _built[family]


def reference_cells():
    """-> (total, per family): DP cells of the distinct (query, target, scheme, open) that the test modules check against the reference - families a to g, the
    reads of family s against their backbones and the checked reads of the large polishing call"""
    seen = set(); per = {}
    for fam in sorted(FAMILIES):
        c = 0
        for case in cases(fam):
            for p in np.nonzero(case.ref)[0]:
                key = (case.queries[case.q_idx[p]], case.targets[case.t_idx[p]], case.match, case.mismatch, int(case.open[p]), case.ext)
                if key not in seen: seen.add(key); c += len(key[0]) * len(key[1])
        per[fam] = c
    per["s"] = sum(len(r) * len(g.backbone) for g in family_s() for r in g.reads)
    many, checked = family_s_many()
    per["s_many"] = sum(len(many.reads[x]) * len(many.backbone) for x in checked)
    return sum(per.values()), per
