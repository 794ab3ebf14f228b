"""Deterministic builders of the edge families of the store pass (ngsid_rec_walk: strand call, oriented copies, the REC instances of k_ed_align) as its five consumers
see it: fixed seeds, plain functions, no tests - the style of ed_cases.py, whose rseq / mutate / spread / other are reused.

Every family_x() returns a list of Case: one Case is ONE call of each consumer - centres, the read set (with qualities), grp_off, read_order, (k, w), clip, a tag per
LISTED read, the sites (phase_genotypes) and the run lists (hp_runs) to ask for.  Every listed entry is a read of its own (a read may be listed under one group only);
repeats are separate reads with the same string, which cost the reference one DP.  The read set is stored in a permuted order, so read_order is never the identity.
Tags: a tuple whose first word names the mechanism; "no_strand" = built to share no minimizer with its centre, "no_column" = built to count no column under the
case's clip.  What a family promises is asserted on the REFERENCE's columns by test_rec_reference_cpu.py, never assumed.

DP cells are those of the distinct oriented (read, centre) pairs; every family stays under ~40 M.
"""
from collections import namedtuple
import numpy as np
from ed_cases import rseq, mutate, spread, other, ACGT
from polish_reference import revcomp

Case = namedtuple("Case", "name desc centres reads quals grp_off read_order k w clip tags site_off site_pos run_off run_start")


def nohp(rng, n):
    """n random letters, no two neighbours equal: an edit at a chosen place has ONE cheapest alignment"""
    out = [ACGT[int(rng.integers(0, 4))]]
    while len(out) < n: out.append(other(rng, out[-1]))
    return "".join(out)


def all_runs(centres):
    """the first positions of all maximal runs of equal letters of every centre -> (run_off, run_start)"""
    off, starts = [0], []
    for c in centres:
        starts += [p for p in range(len(c)) if p == 0 or c[p] != c[p - 1]]
        off.append(len(starts))
    return np.array(off, dtype=np.uint64), np.array(starts, dtype=np.uint32)


def pick_sites(centres, marks):
    """every position of a centre of at most 64 letters; else 0, 7, 8, 63, 64, m - 1, the builder's marks (and their neighbours) and evenly spaced ones, 64 in all"""
    off, pos = [0], []
    for g, c in enumerate(centres):
        m = len(c)
        if m <= 64: s = list(range(m))
        else:
            s = [p for p in (0, 7, 8, 63, 64, m - 1) if p < m]
            for p in marks.get(g, []):
                for d in (0, -1, 1):
                    if 0 <= p + d < m and p + d not in s and len(s) < 56: s.append(p + d)
            for p in np.linspace(0, m - 1, 40).astype(int).tolist():
                if p not in s and len(s) < 64: s.append(p)
            s = sorted(set(s))
        pos += s; off.append(len(pos))
    return np.array(off, dtype=np.uint64), np.array(pos, dtype=np.uint32)


class _Call:
    """collects the groups of one call: centre, listed reads with tags, marked centre positions"""
    def __init__(self):
        self.centres, self.groups, self.marks = [], [], {}

    def group(self, centre, marks=()):
        self.centres.append(centre); self.groups.append([])
        if len(marks): self.marks[len(self.centres) - 1] = list(marks)
        return len(self.centres) - 1

    def read(self, s, tag, times=1, g=-1):
        for _ in range(times): self.groups[g].append((s, tag))

    def mark(self, *pos, g=-1):
        g = g if g >= 0 else len(self.centres) - 1
        self.marks.setdefault(g, []).extend(int(p) for p in pos)

    def case(self, name, desc, k, w, clip, seed):
        listed = [r for grp in self.groups for r in grp]
        nl = len(listed)
        grp_off = np.zeros(len(self.groups) + 1, dtype=np.uint64); grp_off[1:] = np.cumsum([len(grp) for grp in self.groups])
        perm = np.random.default_rng(seed).permutation(nl)              # listed entry x is read perm[x] of the set
        reads = [None] * nl
        for x in range(nl): reads[int(perm[x])] = listed[x][0]
        quals = ["".join(chr(33 + (7 * i + 3 * r + (i * i) % 11) % 94) for i in range(len(s))) for r, s in enumerate(reads)]
        so, sp = pick_sites(self.centres, self.marks); ro, rs_ = all_runs(self.centres)
        return Case(name, desc, list(self.centres), reads, quals, grp_off, perm.astype(np.uint32), k, w, clip, [t for _, t in listed], so, sp, ro, rs_)


def build(pattern, centre, a, rng):
    """a read from the centre, walking from position a: an int L copies L letters, 's' substitutes one, 'd' skips one centre letter, 'i' inserts a letter that differs
    from both neighbours, a string is inserted as it is -> (read, the centre position behind the last letter used)"""
    out, p = [], a
    for it in pattern:
        if isinstance(it, int): out.append(centre[p:p + it]); assert p + it <= len(centre); p += it
        elif it == "s": out.append(other(rng, centre[p])); p += 1
        elif it == "d": p += 1
        elif it == "i": out.append([l for l in ACGT if l != centre[p - 1] and l != centre[p]][0])
        else: out.append(it)
    return "".join(out), p


# ---------------------------------------------------------------------------------------------------------------- r_pack
PACK_LENS = [1, 7, 8, 9, 63, 64, 65, 71, 72, 73, 127, 128, 129, 255, 256, 257, 520]
PACK_SIZE = {1: 1, 63: 63, 65: 65}                # group sizes that make the 64-lane bundles straddle groups


def family_pack():
    """Row packing: ONE call at k = w = 4 with a group per centre length 1, 7, 8, 9, 63, 64, 65, 71, 72, 73, 127, 128, 129, 255, 256, 257, 520 (a dword of the row holds 8
    positions, an 8-byte flush 4 x 4, a row roundup(520, 64) / 8 = 72 dwords: the short rows sit inside the long stride), one empty group and one centre of length 0.
    Per group about 12 reads: the centre, slices that start or end on multiples of 4, 8 and 64 and one off, lightly mutated copies on both strands; homopolymer reads
    (no minimizer after compression: tag no_strand) interleaved, so the pair list shifts against the listed order; groups of 1, 63 and 65 reads.  386 listed reads,
    228 distinct pairs, 7.7 M cells."""
    rng = np.random.default_rng(1101)
    base = nohp(rng, 24) + rseq(rng, 520)
    c = _Call()
    for m in PACK_LENS:
        C = base[:m]
        c.group(C, marks=[p for p in (3, 4, 5, 15, 16, 17, 31, 32, 33, 127, 128, 255, 256, 511, 512) if p < m])
        if m == 1:
            c.read(C, ("no_strand", "one_letter_centre")); continue
        c.read(C, ("equal",))
        cuts = [(0, m - 1), (1, m), (4, m), (0, m - 4), (8, m), (0, m - 8), (5, m - 3), (3, m - 5), (64, m), (0, 64), (1, 65), (63, m), (0, 63), (60, 68), (120, 136)]
        for a, z in cuts:
            if 0 <= a and z <= m and z - a >= 6: c.read(C[a:z], ("slice", a, z))
        c.read("A" * 9, ("no_strand", "homopolymer"))
        if m >= 63:
            for rep in range(2):
                r = mutate(rng, C, 0.03, 0.015, 0.015)
                c.read(r, ("mutated", 0)); c.read(revcomp(r), ("mutated", 1))
            c.read("C" * 5, ("no_strand", "homopolymer"))
            c.read(revcomp(C[2:m - 1]), ("slice_rc", 2, m - 1))
        want = PACK_SIZE.get(m)
        if want:
            k = 0
            while len(c.groups[-1]) < want: c.read(*c.groups[-1][1 + k % 5]); k += 1
            del c.groups[-1][want:]
        if m == 72: c.group(base[100:180])                                       # the empty group
        if m == 128:
            c.group(""); c.read(base[:40], ("no_strand", "empty_centre"), times=3)
    return [c.case("pack", "row packing: centres of %s letters, an empty group, an empty centre" % ", ".join(map(str, PACK_LENS)), 4, 4, False, 11)]


# ---------------------------------------------------------------------------------------------------------------- r_ends
def family_ends():
    """Span ends: ONE call at k = 5, w = 9 with a centre of 130 letters (ACGT) and one of 300 letters that holds three N.  Reads: overhanging the centre on either side
    (leading / trailing 'I'), ending inside the centre on letters the centre does not continue with (an 'I' run behind the last counted column), an inserted base in
    front of the last letter (the INS bit on the second-to-last counted column), a deleted block ('D' run, then '='), N in the read, N in the centre under A / C / G /
    T, N opposite N, and N-only reads around a 60-letter seed.  Both strands.  54 listed reads, 26 distinct pairs, 1.2 M cells."""
    rng = np.random.default_rng(1202)
    c = _Call()
    C1 = nohp(rng, 130)
    C2 = list(nohp(rng, 300))
    for p in (40, 150, 151): C2[p] = "N"
    C2 = "".join(C2)
    for C, name in ((C1, "c130"), (C2, "c300")):
        m = len(C)
        c.group(C, marks=[0, 1, 20, 59, 60, 63, 64, 99, 100, 40, 150, 151, m - 2, m - 1])
        out_l = [l for l in ACGT if l != C[0]]; out_r = [l for l in ACGT if l != C[-1]]
        lead = (out_l[0] + out_l[1]) * 5; trail = (out_r[0] + out_r[1]) * 6
        fam = []
        fam.append((lead + C, ("lead_I",)))
        fam.append((C + trail, ("trail_I",)))
        fam.append((lead + C + trail, ("lead_trail_I",)))
        tail = [l for l in ACGT if l not in C[99:102]][0]              # ends inside the centre on a letter that matches nothing near: X costs what I costs, and the leftmost end column keeps it read-only
        fam.append((C[20:100] + tail, ("I_behind_last",)))
        fam.append((lead[:3] + C[:90], ("I_front_first",)))
        z = 100
        ins = [l for l in ACGT if l not in (C[z - 2], C[z - 1])][0]
        fam.append((C[10:z - 1] + ins + C[z - 1], ("I_behind_second_last",)))
        fam.append((C[:60] + C[64:], ("D_then_eq",)))
        fam.append((C[5:70] + "N" + C[71:125], ("N_in_read",)))
        fam.append((C[:50] + "NN" + C[52:], ("N_in_read",)))
        if "N" in C:
            fam.append((C.replace("N", "A", 1).replace("N", "C", 1).replace("N", "G", 1), ("N_in_centre", "ACG")))
            fam.append((C.replace("N", "T"), ("N_in_centre", "T")))
            fam.append((C, ("N_opposite_N",)))
            fam.append((C[:40] + C[41:], ("N_in_centre_deleted",)))
        fam.append(("N" * 40 + C[60:120] + "N" * 40, ("all_N_but_seed",)))
        fam.append(("N" * 3 + C[60:124] + "N" * 5, ("all_N_but_seed",)))
        for r, tag in fam:
            c.read(r, tag + (0,)); c.read(revcomp(r), tag + (1,))
        c.read("N" * 50, ("no_strand", "all_N"))
    return [c.case("ends", "span ends: leading / trailing I, the INS bit at the last columns, D runs, N on either side", 5, 9, False, 12)]


# ---------------------------------------------------------------------------------------------------------------- r_ties
TIE_TOTAL = [63, 64, 65, 127, 128, 129]


def family_ties():
    """The tie rule as the consumers see it: ONE call at k = 5, w = 9; a group per repeat - a homopolymer of 2 ... 20 letters, AC x 2, 3, 5, 8, 10 and ACG x 2, 3, 5, 7 -
    between random flanks, the centre 63, 64, 65, 127, 128 or 129 letters long in turn, with reads whose repeat is one or two letters shorter or longer (which centre
    position carries the 'D', which the INS bit, is decided by diagonal first, then read-only, then centre-only) and the equal read, both strands; and three centres
    that hold a read twice (the leftmost end column wins), and three where read-only and centre-only continue a cheapest path and no diagonal does.  295 listed reads,
    146 distinct pairs, 1.4 M cells."""
    rng = np.random.default_rng(1303)
    c = _Call()
    units = [("A", n) for n in range(2, 21)] + [("AC", n) for n in (2, 3, 5, 8, 10)] + [("ACG", n) for n in (2, 3, 5, 7)]
    for x, (u, n) in enumerate(units):
        unit = u if x % 2 == 0 or len(u) > 1 else "T"
        rep = unit * n
        total = TIE_TOTAL[x % 6]
        fl = (total - len(rep)) // 2; fr = total - len(rep) - fl
        L = nohp(rng, fl); R = nohp(rng, fr)
        if L[-1] == rep[0]: L = L[:-1] + [l for l in ACGT if l not in (rep[0], L[-2])][0]
        if R[0] == rep[-1]: R = [l for l in ACGT if l not in (rep[-1], R[1])][0] + R[1:]
        C = L + rep + R
        c.group(C, marks=[fl - 1, fl, fl + 1, fl + len(rep) - 2, fl + len(rep) - 1, fl + len(rep)])
        for d in (0, -2, -1, 1, 2):
            body = (unit * (n + 2))[:len(rep) + d] if d >= 0 else rep[:len(rep) + d]
            r = L + body + R
            c.read(r, ("repeat", unit, n, d, 0)); c.read(revcomp(r), ("repeat", unit, n, d, 1))
    for n, gap in ((45, 0), (50, 1), (60, 30)):
        Q = nohp(rng, n)
        C = nohp(rng, 17) + Q + nohp(rng, gap) + Q + nohp(rng, 9)
        c.group(C, marks=[16, 17, 17 + n - 1, 17 + n])
        c.read(Q, ("twice", n, gap, 0), times=2); c.read(revcomp(Q), ("twice", n, gap, 1))
    # read-only or centre-only: the centre holds "aba" where the read starts with "ab" - "a" on the second a and b read-only, or "ab" on "ab" and the second a
    # centre-only, cost the same, and no diagonal column continues a cheapest path from that cell: the only rule left is read-only first
    for (a, b), pre, total in ((("A", "C"), 20, 64), (("G", "T"), 31, 65), (("T", "A"), 60, 128)):
        P = nohp(rng, pre); R = nohp(rng, total - pre - 3)
        if P[-1] in (a, b): P = P[:-1] + [l for l in ACGT if l not in (a, b, P[-2])][0]
        if R[0] in (a, b): R = [l for l in ACGT if l not in (a, b, R[1])][0] + R[1:]
        c.group(P + a + b + a + R, marks=[pre, pre + 1, pre + 2, pre + 3])
        r = a + b + R[:total - pre - 8]
        c.read(r, ("up_or_left", a + b, pre, 0)); c.read(revcomp(r), ("up_or_left", a + b, pre, 1))
    return [c.case("ties", "ties: homopolymers of 2 - 20, AC and ACG tandems, reads one or two letters short or long, a read that occurs twice", 5, 9, False, 13)]


# ---------------------------------------------------------------------------------------------------------------- r_clip
CLIP_PATTERNS = [
    ("head_run", 14, [14, "s", 5, "s", 40, "s", 30]),
    ("head_run", 15, [15, "s", 5, "s", 40, "s", 30]),
    ("head_run", 16, [16, "s", 5, "s", 40, "s", 30]),
    ("tail_run", 14, [30, "s", 40, "s", 5, "s", 14]),
    ("tail_run", 15, [30, "s", 40, "s", 5, "s", 15]),
    ("tail_run", 16, [30, "s", 40, "s", 5, "s", 16]),
    ("single_run", 15, [8, "s", 9, "s", 15, "s", 10, "s", 7]),
    ("single_run_gap", 15, [8, "d", 9, "i", 15, "d", 10, "i", 7]),
    ("start_run", 20, [20, "s", 9, "s", 11, "s", 4]),
    ("no_run", 0, [10, "s", 14, "s", 12, "d", 14, "i", 13, "s", 9]),
    ("ended_by_gap", 15, [6, "s", 15, "d", 12, "s", 16, "i", 8, "s", 15, "i", 6]),
    ("ended_by_X", 15, [6, "i", 15, "s", 12, "d", 16, "s", 8, "d", 15, "s", 6]),
    ("edits_outside", 0, [5, "i", 6, "d", 8, "s", 30, "s", 25, "s", 7, "d", 6, "i", 5]),
    ("ins_before_first_run", 0, [10, "i", 40, "s", 20]),
    ("ins_before_first_run", 1, [10, "s", 3, "i", 15, "d", 40, "i", 15, "i", 8]),
    ("overhang", 0, ["GGTTGGTTAACC", 60, "s", 20, "CCAACCAATTGG"]),
]


def family_clip():
    """The CLIP + REC instance: the same groups called with clip = 1 and with clip = 0 (contrast), k = w = 5 (every 5-mer is a minimizer: reads cut into short runs keep their strand), centres of 260 letters without equal neighbours (an
    edit has one cheapest alignment).  Reads walk the centre from position 10 or 3: equal runs of exactly 14, 15 and 16 columns at the head and at the tail, a single
    run of 15 (ended by X, and by gaps), a run of 20 that holds the read's start, no run at all (tag no_column under clip = 1), runs ended by X and by a gap, edits
    and I / D in the clipped-off head and tail, an inserted base directly in front of the first run (the INS bit of the first counted column's predecessor), and
    overhangs.  Both strands, two centres.  128 listed reads and 64 distinct pairs per call (the same in both), 1.4 M cells."""
    out = []
    for clip in (True, False):
        rng = np.random.default_rng(1404)
        c = _Call()
        for g in range(2):
            C = nohp(rng, 260)
            c.group(C, marks=[9, 10, 11, 24, 25, 26])
            for a in (10, 3):
                for name, L, pat in CLIP_PATTERNS:
                    r, z = build(pat, C, a, rng)
                    tag = ("no_column", name) if (clip and name == "no_run") else (name, L, a)
                    c.read(r, tag + (0,)); c.read(revcomp(r), tag + (1,))
                    c.mark(a + 14, a + 15, a + 16, z - 16, z - 15, z - 1, z)
        out.append(c.case("clip%d" % clip, "runs of 14 / 15 / 16 equal columns at either end, one run, no run, edits outside the runs; clip = %d" % clip, 5, 5, clip, 14))
    return out


# ---------------------------------------------------------------------------------------------------------------- r_inst
INST_LENS = [256, 257, 512, 513, 768, 769, 896, 897, 1024, 1025, 2752, 2784]


def family_inst():
    """Instance selection, clip = 0, k = 13, w = 20: one call per longest read 256, 257, 512, 513, 768, 769, 896, 897, 1024, 1025, 2752, 2784 (the longest read of the
    read set selects the instance).  Two centres; 3 distinct reads at 1, 2 and 3 % error - one of exactly the length, the others a little shorter (700 letters
    in the two longest calls, to stay under the cap) - copied over a bundle and a half (96 listed reads, alternating strands), plus one 60-letter slice bundled with the
    long ones.  4 distinct oriented pairs per call (the two strands orient to the same strings); 1 152 listed reads and 48 distinct pairs in the twelve calls; cells: 2 x (0.2 + 0.8 + 1.8 + 2.5 + 3.2) M + 2 x 10.4 M = 37.9 M."""
    out = []
    for x, n in enumerate(INST_LENS):
        rng = np.random.default_rng(1500 + n)
        c = _Call()
        other_len = [n - 9, n - 30] if n < 2000 else [700, 690]
        CA = rseq(rng, n + 24); CB = rseq(rng, other_len[1] + 40)
        def rd(C, L, err):
            return (mutate(rng, C[3:], err * 0.4, err * 0.3, err * 0.3) + rseq(rng, 64))[:L]
        r0, r1, r2 = rd(CA, n, 0.01), rd(CA, other_len[0], 0.02), rd(CB, other_len[1], 0.03)
        c.group(CA, marks=[255, 256, 511, 512, 767, 768, 895, 896, 1023, 1024])
        for y in range(64):
            r = (r0, r1)[y % 3 == 1]
            c.read(revcomp(r) if y % 2 else r, ("long", len(r), y % 2))
            if y == 40: c.read(CA[n // 2:n // 2 + 60], ("short_slice", 60, 0))
        c.group(CB, marks=[255, 256, 511, 512, 767, 768])
        for y in range(31): c.read(revcomp(r2) if y % 2 else r2, ("long", len(r2), y % 2))
        out.append(c.case("inst%d" % n, "longest read %d letters, 96 listed reads of 3 distinct ones + a 60-letter slice" % n, 13, 20, False, 15 + x))
    return out


# ---------------------------------------------------------------------------------------------------------------- r_band
BAND_KS = [12, 40, 150]
BAND_FLANK = {12: 70, 40: 150, 150: 320}           # as ed_cases.family_b: longer than the 2K block, and the longest read selects the 4-, 8-, 16-block instance
BAND_CAP = {12: 256, 40: 512, 150: 1024}


def family_band():
    """Distance around a band K, clip = 0, k = 13, w = 20: per K in 12, 40, 150 one call with, for L in K - 1, K, K + 1, 2K: L edits spread evenly between two clean
    60-letter flanks (so the read keeps minimizers: it gets a strand) - insertion-heavy and deletion-heavy; ONE block of L inserted read letters; ONE block of L
    deleted centre letters (ed_cases.family_b's constructions).  Every distinct pair is a group of its own: first one read each (one mixed bundle, the last group
    padded to 64 pairs), then 64 copies each (a bundle of its own: the band's lower edge is the wave-wide minimum of n - m).  15 distinct pairs and 1 024 listed reads
    per K; cells 0.3 + 1.8 + 9.1 = 11.2 M."""
    out = []
    for K in BAND_KS:
        rng = np.random.default_rng(1600 + K)
        F = BAND_FLANK[K]
        T = rseq(rng, 2 * F + 2 * K - 20)
        S = T[:BAND_CAP[K] - (4 * K) // 3 - 4]
        pairs = []
        lens = [K - 1, K, K + 1, 2 * K]
        for L in lens:
            for heavy in ("i", "d"):
                if L == 2 * K and heavy == "d": continue
                kinds = [heavy if x % 3 != 2 else "s" for x in range(L)]
                pairs.append((S[:60] + spread(rng, S[60:-60], kinds) + S[-60:], S, ("spread", K, L, heavy)))
        A, Cc = T[:F], T[F:2 * F]
        for L in lens:
            pairs.append((A + rseq(rng, L) + Cc, A + Cc, ("qblock", K, L)))
        for L in lens:
            pairs.append((A + Cc, A + rseq(rng, L) + Cc, ("tblock", K, L)))
        c = _Call()
        for x, (r, C, tag) in enumerate(pairs):
            c.group(C); c.read(r if x % 2 == 0 else revcomp(r), tag + (x % 2,), times=1 if x < len(pairs) - 1 else 64 - (len(pairs) - 1))
        for x, (r, C, tag) in enumerate(pairs):
            c.group(C); c.read(r if x % 2 == 0 else revcomp(r), tag + (x % 2,), times=64)
        assert max(len(r) for r, _, _ in pairs) <= BAND_CAP[K]
        out.append(c.case("band%d" % K, "distances K-1, K, K+1, ~2K around K = %d: spread edits, one read block, one centre block" % K, 13, 20, False, 16 + K))
    return out


# ---------------------------------------------------------------------------------------------------------------- r_class
CLASSES = [(60, 256), (257, 512), (513, 768), (769, 896), (897, 1024)]


def _class_pairs(rng):
    """8 distinct (read, centre) pairs per length class: 5 at 1 - 2 % error, the class's shortest and longest read, and one with a block of 110 / 140 / 215 inserted
    letters where the class has room for flanks longer than the block (else one more low-error pair): distances on both sides of the default band of 64 + 1024 / 32"""
    per = []
    for ci, (lo, top) in enumerate(CLASSES):
        pairs = []
        for k in range(8):
            L = (110, 140, 215, 110, 215)[ci]
            if k == 7 and top >= 3 * L + 20:
                n = top - 3; T = rseq(rng, n - L + 8); h = (n - L) // 2
                r = (T[:h] + rseq(rng, L) + T[h:])[:n]
                pairs.append((r, T, ("class_block", ci, L)))
                continue
            n = top if k == 6 else lo if k == 5 else int(rng.integers(lo, top + 1))
            T = rseq(rng, n + int(rng.integers(0, 25)))
            r = (mutate(rng, T[int(rng.integers(0, 5)):], 0.01, 0.005, 0.005) + rseq(rng, 40))[:n]
            pairs.append((r, T, ("class", ci, n)))
        per.append(pairs)
    return per


def family_class():
    """Class launches, clip = 0, k = 13, w = 20: 4 096 and 4 097 listed reads as copies of 40 distinct reads, 8 per length class (<= 256, 257 - 512, 513 - 768, 769 - 896,
    > 896; centres of at most 1 050 letters), every distinct pair a group, the groups in an order that mixes the classes, group sizes of about 100 (so every bundle
    straddles groups of two classes); variants with no read in 513 - 768, none in 769 - 896 and none above 896.  Every read has a strand (the class launches start at
    4 096 PAIRS).  Four pairs hold an inserted block of 110, 140 or 215 letters: beyond the default band, and (two of them, in 513 - 768 and above 896) beyond the retry launch's 180.  20 482 listed reads in the five calls, 40 distinct pairs, 17.6 M cells."""
    rng = np.random.default_rng(1707)
    per = _class_pairs(rng)
    out = []
    for name, n, drop in (("class4096", 4096, None), ("class4097", 4097, None), ("class_no_513_768", 4096, 2), ("class_no_769_896", 4097, 3), ("class_no_gt896", 4096, 4)):
        pairs = [per[ci][k] for k in range(8) for ci in range(5) if ci != drop]
        c = _Call()
        sizes = np.full(len(pairs), n // len(pairs)); sizes[:n - int(sizes.sum())] += 1
        for j in range(0, len(pairs) - 1, 2): sizes[j] += 5 + 3 * (j % 7); sizes[j + 1] -= 5 + 3 * (j % 7)      # no group boundary on a bundle boundary
        for x, ((r, T, tag), s) in enumerate(zip(pairs, sizes.tolist())):
            c.group(T, marks=[255, 256, 511, 512, 767, 768, 895, 896])
            for y in range(s): c.read(revcomp(r) if (x + y) % 2 else r, tag + ((x + y) % 2,))
        assert sum(len(g) for g in c.groups) == n
        out.append(c.case(name, "%d listed reads over %d distinct ones%s" % (n, len(pairs), "" if drop is None else ", class %d - %d empty" % CLASSES[drop]), 13, 20, False, 17 + n))
    return out


FAMILIES = {"pack": family_pack, "ends": family_ends, "ties": family_ties, "clip": family_clip, "inst": family_inst, "band": family_band, "class": family_class}
_built = {}


def cases(family):
    """the (cached) cases of one family"""
    if family not in _built: _built[family] = FAMILIES[family]()
    return _built[family]
