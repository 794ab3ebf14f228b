"""Deterministic builders of the edge families of the edit-distance aligner (k_ed_align): fixed seeds, plain functions, no tests.

Every family_x() returns a list of Case: one Case is one call of ed_align_batch - (queries, targets, q_idx, t_idx, window, bp_windows) plus
a name, a description and `tags` (what the builder intended per distinct pair, for the family conditions of test_ed_reference_cpu.py,
which are asserted on the REFERENCE's results, never assumed).  The instance of the kernel is chosen per CALL by the longest query, so a
family that aims at several instances is several calls.  Pairs repeated by index cost the reference one DP (ed_reference deduplicates),
so whole 64-lane bundles of one pair are cheap.  DP cells (distinct pairs, n x m) are stated per family; the cap is ~60 M.
"""
from collections import namedtuple
import numpy as np

Case = namedtuple("Case", "name desc queries targets q_idx t_idx window bp_windows tags")
ACGT = "ACGT"


def rseq(rng, n):
    return "".join(ACGT[x] for x in rng.integers(0, 4, n))


def other(rng, ch):
    return ACGT[(ACGT.index(ch) + int(rng.integers(1, 4))) % 4]


def mutate(rng, s, sub, ins, dele):
    out = []
    for ch in s:
        u = rng.random()
        if u < dele: continue
        if u < dele + ins: out.append(ACGT[rng.integers(0, 4)])
        out.append(other(rng, ch) if rng.random() < sub else ch)
    return "".join(out)


def spread(rng, s, kinds):
    """len(kinds) edits ('s' substitution, 'i' inserted base, 'd' deleted base) at evenly spaced positions of s"""
    s = list(s); e = len(kinds)
    pos = [int((k + 0.5) * len(s) / e) for k in range(e)]
    for k in reversed(range(e)):
        p = pos[k]
        if kinds[k] == "s": s[p] = other(rng, s[p])
        elif kinds[k] == "d": del s[p]
        else: s.insert(p, other(rng, s[p]))            # differs from the base that follows it: no free slide into a match
    return "".join(s)


class _Build:
    """collects distinct sequences and pairs of one call"""
    def __init__(self):
        self.q, self.t, self.qi, self.ti, self.tags = [], [], [], [], []
        self._q, self._t = {}, {}

    def qid(self, s):
        if s not in self._q: self._q[s] = len(self.q); self.q.append(s)
        return self._q[s]

    def tid(self, s):
        if s not in self._t: self._t[s] = len(self.t); self.t.append(s)
        return self._t[s]

    def pair(self, q, t, tag=None, times=1):
        a, b = self.qid(q), self.tid(t)
        for _ in range(times):
            self.qi.append(a); self.ti.append(b); self.tags.append(tag)

    def pad_bundle(self):
        """repeat the last pair up to the next multiple of 64, so that what follows starts a bundle of its own"""
        while len(self.qi) % 64: self.qi.append(self.qi[-1]); self.ti.append(self.ti[-1]); self.tags.append(self.tags[-1])

    def case(self, name, desc, window=100, bp_windows=None, order=None):
        qi = np.array(self.qi, dtype=np.uint32); ti = np.array(self.ti, dtype=np.uint32); tags = list(self.tags)
        if order is not None: qi, ti, tags = qi[order], ti[order], [tags[k] for k in order]
        if bp_windows is None: bp_windows = (max([len(x) for x in self.t] + [1]) + window - 1) // window
        return Case(name, desc, list(self.q), list(self.t), qi, ti, window, bp_windows, tags)


# ---------------------------------------------------------------------------------------------------------------- a
A_QLENS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, 768, 769, 895, 896, 897, 1023, 1024, 1025, 1087, 1088, 1089]
A_GROUPS = [256, 512, 768, 1024, 1 << 30]          # one call per instance: 4, 8, 12, 16 blocks and block groups / the sliding window


def family_a():
    """Block and launch boundaries.  Per query length n: three lightly mutated slices of a target with target lengths n + d (d rotating
    through -9 ... +9 over the lengths, every d used), one unrelated sequence against a target of length n + d, and related + unrelated
    against targets of 1, 63, 64, 65 and 0 bases.  ~11.9 M cells (sum of n^2) x 4 near-length pairs + ~3 M = ~51 M cells, 14 per length."""
    rng = np.random.default_rng(101)
    deltas = list(range(-9, 10))
    base = rseq(rng, 1200)
    out = []; k = 0
    for g, hi in enumerate(A_GROUPS):
        lo = A_GROUPS[g - 1] if g else 0
        b = _Build()
        for n in [x for x in A_QLENS if lo < x <= hi]:
            for rep in range(4):
                d = deltas[k % len(deltas)]; k += 7
                m = max(n + d, 0)
                T = base[5:5 + m]
                if rep < 3:
                    src = T[:n] if d >= 0 else T + rseq(rng, -d)        # d < 0: the query overhangs the target by -d bases
                    q = mutate(rng, src, 0.02, 0.01, 0.01)
                    q = (q + rseq(rng, n))[:n]
                else:
                    q = rseq(rng, n)
                b.pair(q, T, ("near", n, d, rep < 3))
            rel = (mutate(rng, base[40:40 + n], 0.02, 0.01, 0.01) + rseq(rng, 8))[:n]
            unrel = rseq(rng, n)
            for m in (1, 63, 64, 65, 0):
                b.pair(rel, base[40:40 + m], ("short_target", n, m, True))
                b.pair(unrel, base[40:40 + m], ("short_target", n, m, False))
        out.append(b.case("a_le%d" % hi if hi < (1 << 30) else "a_gt1024", "block boundaries, queries of %d < n <= %s bases" % (lo, hi if hi < (1 << 30) else "1089")))
    return out


# ---------------------------------------------------------------------------------------------------------------- b
B_KS = [12, 40, 100, 150, 180]
# flank length per K: longer than the 2K block (clipping a flank must not be cheaper than the block), and such that the longest query of the
# call selects the 4-, 8-, 12-, 16-block instance and (K = 180) the sliding-window one
B_FLANK = {12: 60, 40: 150, 100: 250, 150: 320, 180: 400}
B_CAP = {12: 256, 40: 512, 100: 768, 150: 1024}       # longest query of the call


def family_b():
    """Distance around a band K: per K one call with, for L in K-1, K, K+1, 2K: (1) L edits spread evenly - insertion-heavy (n > m) and
    deletion-heavy (n < m); (2) ONE block of L inserted query bases mid-read, against the bare target (n > m, the path ends on diagonal +L)
    and against the target with a prefix flank (n < m, the path runs on the band's lower edge); (3) ONE block of L deleted target bases
    (n < m).  The first bundle holds every distinct pair once (mixed n - m), then every pair fills a bundle of its own (the band's lower
    edge is the wave-wide minimum of n - m: only a uniform bundle has the tight band).  A 2K block between flanks that still fit the call's
    instance is cheaper to clip than to bridge - the reference says what came out (test_ed_reference_cpu.py asserts K-1, K, K+1 per
    construction).  19 distinct pairs per K, ~43 M cells."""
    rng = np.random.default_rng(202)
    out = []
    for K in B_KS:
        F = B_FLANK[K]
        b = _Build()
        T = rseq(rng, 2 * F + 2 * K - 20)
        S = T[:B_CAP[K] - (4 * K) // 3 - 4] if K in B_CAP else T        # the insertion-heavy 2K read must not leave the instance the call aims at
        lens = [K - 1, K, K + 1, 2 * K]
        for L in lens:
            for heavy in ("i", "d"):
                if L == 2 * K and heavy == "d": continue
                kinds = [heavy if x % 3 != 2 else "s" for x in range(L)]
                b.pair(spread(rng, S, kinds), S, ("spread", K, L, heavy))
        A, C = T[:F], T[F:2 * F]
        pre = rseq(rng, 2 * K + 40)
        for L in lens:
            blk = rseq(rng, L)
            b.pair(A + blk + C, A + C, ("qblock", K, L, "bare"))
            b.pair(A + blk + C, pre + A + C, ("qblock", K, L, "prefix"))
        for L in lens:
            blk = rseq(rng, L)
            b.pair(A + C, A + blk + C, ("tblock", K, L, None))
        ndist = len(b.qi)
        b.pad_bundle()
        for k in range(ndist):
            b.pair(b.q[b.qi[k]], b.t[b.ti[k]], b.tags[k], times=64)
        out.append(b.case("b_K%d" % K, "distances K-1, K, K+1, ~2K around K = %d: spread edits, one query block, one target block" % K))
    return out


# ---------------------------------------------------------------------------------------------------------------- c
def _c_content(rng, top):
    """64 pairs: the six edge pairs + 58 lanes over 12 distinct full-length low-error pairs of 700 ... top bases"""
    edge, full = [], []
    T15 = rseq(rng, 1500)
    edge.append(("", rseq(rng, 800), "empty_query"))
    edge.append(("G", rseq(rng, 900), "one_base"))
    edge.append((mutate(rng, T15[700:730], 0.05, 0.0, 0.0), T15, "short_in_long"))
    T6 = rseq(rng, 600)
    edge.append((T6[:300] + rseq(rng, 200) + T6[300:], T6, "query_200_longer"))
    edge.append((rseq(rng, 750), "", "empty_target"))
    edge.append((rseq(rng, 40), rseq(rng, 64), "unrelated_short"))
    for k in range(12):
        L = 700 + (top - 700) * k // 11
        T = rseq(rng, L + int(rng.integers(0, 12)))
        full.append((mutate(rng, T[int(rng.integers(0, 6)):], 0.015, 0.008, 0.008)[:L], T, "full"))
    return edge, full


def family_c():
    """Mixed bundles: the band's dmin, nmax and mmax are wave-wide.  One 64-pair content (empty query, 1-base query, 30 bases inside 1 500,
    a query 200 bases longer than its target, an empty target, 12 distinct full-length pairs of 700 - 1 000 bases on the other lanes by
    repeated, non-identity indices) in three lane orders - edge pairs from lane 0, up to lane 63, shuffled - and cut / extended to 1, 63,
    65 and 129 pairs; the same with full-length pairs up to 1 100 bases (longest query > 1 024: the sliding-window instance, whose
    window-span check sends such a wave to the unbanded launch).  Cells: 2 x (12 x ~0.8 M + ~0.5 M) = ~21 M."""
    out = []
    for top, seed in ((1000, 303), (1100, 304)):
        rng = np.random.default_rng(seed)
        edge, full = _c_content(rng, top)
        b = _Build()
        for q, t, tag in edge: b.pair(q, t, tag)
        for k in range(58): q, t, tag = full[(k * 5) % 12]; b.pair(q, t, tag)
        first = np.arange(64); last = np.concatenate([np.arange(6, 64), np.arange(6)[::-1]])
        shuf = np.random.default_rng(seed + 10).permutation(64)
        sfx = "_top%d" % top
        out.append(b.case("c_lane0" + sfx, "mixed bundle, edge pairs in lanes 0-5", order=first))
        out.append(b.case("c_lane63" + sfx, "mixed bundle, edge pairs in lanes 58-63 (empty query in lane 63)", order=last))
        out.append(b.case("c_shuffled" + sfx, "mixed bundle, shuffled lanes", order=shuf))
        for n in (1, 63, 65, 129):
            order = np.concatenate([last, shuf, first])[:n] if n > 1 else np.array([2])
            out.append(b.case("c_%dpairs%s" % (n, sfx), "mixed content, %d pairs" % n, order=order))
    return out


# ---------------------------------------------------------------------------------------------------------------- d
def family_d():
    """Ties: homopolymers, di- and tri-nucleotide repeats, a query that occurs several times in its target (leftmost end wins), a query
    of Ns, lower and mixed case, N / IUPAC letters in the query, in the target and opposite each other; lengths around 64, 128 and 700.
    ~40 pairs, ~9 M cells."""
    rng = np.random.default_rng(404)
    b = _Build()
    for n, m in ((64, 128), (65, 63), (63, 64), (128, 129), (129, 700), (700, 705)):
        b.pair("A" * n, "A" * m, "homopolymer")
    b.pair("A" * 64, "C" * 30 + "A" * 200, "homopolymer_offset")
    b.pair("A" * 700, "A" * 690 + "C" + "A" * 50, "homopolymer_break")
    b.pair("T" * 128, "T" * 60 + "G" + "T" * 60 + "G" + "T" * 200, "homopolymer_break")
    for unit in ("AC", "ACG"):
        for n, m in ((64, 130), (128, 256), (700, 720)):
            rep = unit * (m // len(unit) + 2)
            b.pair(rep[:n], rep[:m], "tandem")
            b.pair(rep[1:n // 2] + rep[n // 2 + 1:n + 2], rep[:m], "tandem_deleted_base")       # which unit of the repeat is missing is a tie
            b.pair(rep[:n // 2] + unit[0] + rep[n // 2:n], rep[:m], "tandem_inserted_base")
    for n, gap in ((64, 10), (128, 1), (200, 30)):
        q = rseq(rng, n)
        b.pair(q, rseq(rng, 17) + q + rseq(rng, gap) + q + rseq(rng, gap) + q + rseq(rng, 9), "exact_copies")
    b.pair("ACGTTGCA" * 8, "ACGTTGCA" * 30, "exact_copies")
    for n, m in ((64, 128), (128, 64), (700, 700)):
        b.pair("N" * n, rseq(rng, m), "all_N")
    b.pair("N" * 64, "N" * 128, "all_N")
    T = rseq(rng, 700)
    b.pair(T[100:228].lower(), T, "case"); b.pair(T[100:228], T.lower(), "case")
    mixed = "".join(c.lower() if rng.random() < 0.5 else c for c in T[5:695])
    b.pair(mixed, T, "case"); b.pair(mixed, "".join(c.lower() if rng.random() < 0.5 else c for c in T), "case")
    iupac = "NRYKMSWBDHVnry"
    def sprinkle(s, k):
        s = list(s)
        for p in rng.choice(len(s), k, replace=False): s[p] = iupac[rng.integers(0, len(iupac))]
        return "".join(s)
    for a, z in ((300, 364), (200, 328), (0, 700)):
        qn = sprinkle(T[a:z], max(2, (z - a) // 20)); tn = sprinkle(T, 40)
        b.pair(qn, T, "iupac_query"); b.pair(T[a:z], tn, "iupac_target")
        tl = list(tn); ql = list(T[a:z])
        for p in range(a, z):
            if tl[p] not in ACGT: ql[p - a] = tl[p]                      # the same non-ACGT letter on both sides: still a mismatch
        b.pair("".join(ql), tn, "iupac_opposite")
    return [b.case("d_ties", "ties: repeats, copies, N, case, IUPAC", window=64)]


# ---------------------------------------------------------------------------------------------------------------- e
E_WINDOWS = [1, 7, 64, 100, 500, 5000]


def family_e():
    """Break points: one set of pairs under window = 1, 7, 64, 100, 500 and one larger than every target, each with bp_windows smaller
    than, equal to and larger than the number of windows of the longest target.  The pairs: exact slices that start / end exactly on the
    boundaries of each window size (and one base off), a slice over the whole target, lightly mutated reads, and for each window size a
    read whose deleted block covers exactly one or two whole windows between aligned flanks (all -1 strictly inside).  Cells ~31 M."""
    rng = np.random.default_rng(505)
    b = _Build()
    T = rseq(rng, 700); T2 = rseq(rng, 3200)
    gaps, gaps2 = ((300, 400), (256, 320), (140, 161), (300, 301)), ((1024, 1152), (1500, 2000))
    for a, z in ((100, 300), (99, 301), (101, 299), (64, 128), (63, 129), (7, 14), (0, 700), (0, 500), (500, 700), (499, 501), (128, 129)):
        b.pair(T[a:z], T, ("slice", a, z))
    b.pair(mutate(rng, T, 0.03, 0.01, 0.01), T, ("read",))
    b.pair(mutate(rng, T[150:650], 0.03, 0.02, 0.02), T, ("read",))
    b.pair(mutate(rng, T2[100:2100], 0.02, 0.01, 0.01), T2, ("read",))
    b.pair(T2[500:1000], T2, ("slice", 500, 1000))
    # A deleted block of RANDOM bases is not one gap: the read's bases beside it match a subsequence of the block for free, and the traceback, which prefers
    # diagonals, scatters the gap.  A block of N in the target matches nothing: the whole block is gap columns, its windows stay empty.
    for S, gs in ((T, gaps), (T2, gaps2)):
        for a, z in gs:
            b.pair(S[:a] + S[z:], S[:a] + "N" * (z - a) + S[z:], ("gap", a, z))
    b.pair("", T, ("empty",)); b.pair(rseq(rng, 50), T2, ("unrelated",))
    out = []
    for W in E_WINDOWS:
        nw = (3200 + W - 1) // W
        for nm, k in (("fewer", max(1, nw // 2)), ("equal", nw), ("more", nw + 3)):
            if nm == "fewer" and nw == 1: continue
            out.append(b.case("e_w%d_%s" % (W, nm), "window %d, bp_windows %d (%s than the %d windows)" % (W, k, nm, nw), window=W, bp_windows=k))
    return out


# ---------------------------------------------------------------------------------------------------------------- f
F_QLENS = [1025, 2049, 2752, 2753, 2754, 2784, 4100]     # 2 752 / 2 784: where 64 + n / 32 passes 150 (the 16-block window takes over)


def family_f():
    """Long reads: one call per query length (the instance is chosen by the longest query of a call) - 1 025, 2 049, 2 752, 2 753, 2 754,
    2 784, 4 100 - against a target of similar length at 1 - 3 % error, the pair repeated over a bundle and a half, plus the 2 049 pair
    bundled with a 30-base query inside the same long target (the window-span check sends that wave to the fallback).  ONE distinct pair
    per length: the repeats the issue allows ('a few pairs each') are dropped to stay under the cap - 1.1 + 4.2 + 4 x 7.7 + 16.9 = ~53 M
    cells."""
    rng = np.random.default_rng(606)
    out = []; keep = None
    for k, n in enumerate(F_QLENS):
        T = rseq(rng, n + 30 + 7 * k)
        err = 0.01 + 0.02 * (k % 3) / 2
        q = (mutate(rng, T[3:], err * 0.5, err * 0.25, err * 0.25) + rseq(rng, 64))[:n]
        b = _Build(); b.pair(q, T, ("long", n), times=70 if n < 4100 else 3)
        out.append(b.case("f_%d" % n, "long read, %d bases at %.1f %% error" % (n, 100 * err), window=500))
        if n == 2049: keep = (q, T)
    b = _Build()
    b.pair(keep[0], keep[1], ("long", 2049), times=20); b.pair(keep[1][900:930], keep[1], ("short_in_long",)); b.pair(keep[0], keep[1], ("long", 2049), times=50)
    out.append(b.case("f_mixed", "2 049-base reads bundled with a 30-base query inside the 2 100-base target", window=500))
    return out


# ---------------------------------------------------------------------------------------------------------------- g
G_CLASSES = [(1, 256), (257, 512), (513, 768), (769, 896), (897, 1024)]


def _g_pairs(rng):
    """12 distinct pairs per query-length class: 9 low-error ones (two of them with the class's shortest and longest query), 2 with a block of
    110 / 140 inserted bases (a distance between the default band and 180) and 1 with a block of 215 (above 180); a class too short for a
    block with longer flanks gets an unrelated query of nearly its top length instead"""
    def block_pair(n, L):
        T = rseq(rng, n - L + 8); h = (n - L) // 2
        return (T[:h] + rseq(rng, L) + T[h:])[:n], T
    per = []
    for c, (lo, top) in enumerate(G_CLASSES):
        pairs = []
        for k in range(12):
            if k in (7, 8, 9):
                L = 215 if k == 9 else 110 + 30 * (k - 7); n = top - k
                q, T = block_pair(n, L) if top >= 3 * L + 20 else (rseq(rng, n), rseq(rng, n + 10))
            else:
                n = top if k == 11 else lo if k == 10 else int(rng.integers(max(lo, 60), top + 1))
                T = rseq(rng, n + int(rng.integers(0, 25)))
                q = (mutate(rng, T[int(rng.integers(0, 5)):], 0.01, 0.005, 0.005) + rseq(rng, 40))[:n]
            assert lo <= len(q) <= top
            pairs.append((q, T, ("class", c)))
        per.append(pairs)
    return per


def family_g():
    """Class launches: 4 096 and 4 097 pairs made by indexing 60 distinct (query, target) pairs, 12 per query-length class (<= 256, 257-512,
    513-768, 769-896, > 896), in shuffled order; variants with no pair in 513-768, none in 769-896, none above 896, and one whose longest
    query has 1 100 bases (the top class then runs in the sliding-window instance).  Distances on both sides of the default band, in
    (band, 180] and above 180: the retry launch and the unbanded launch both get work.  Cells ~0.3 + 2 + 5 + 8.5 + 11 (+ 3 for the
    1 100-base variant) = ~30 M."""
    rng = np.random.default_rng(707)
    per = _g_pairs(rng)
    longer = [(mutate(rng, T, 0.01, 0.005, 0.005)[:1100], T, ("class", 4)) for T in (rseq(rng, 1110), rseq(rng, 1120))]
    out = []
    for name, n, drop, extra in (("g_4096", 4096, None, []), ("g_4097", 4097, None, []), ("g_no_513_768", 4096, 2, []), ("g_no_769_896", 4097, 3, []),
                                 ("g_no_gt896", 4096, 4, []), ("g_top1100", 4096, None, longer)):
        b = _Build()
        for c in range(5):
            if c != drop:
                for q, t, tag in per[c]: b.pair(q, t, tag)
        for q, t, tag in extra: b.pair(q, t, tag)
        nd = len(b.qi)
        order = np.random.default_rng(700 + n + (drop or 0)).integers(0, nd, n); order[:nd] = np.random.default_rng(1).permutation(nd)       # every distinct pair at least once
        out.append(b.case(name, "%d pairs over %d distinct ones%s" % (n, nd, "" if drop is None else ", class %d-%d empty" % G_CLASSES[drop]), order=order))
    return out


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e, "f": family_f, "g": family_g}
_built = {}


def cases(family):
    """the (cached) cases of one family"""
    if family not in _built: _built[family] = FAMILIES[family]()
    return _built[family]
