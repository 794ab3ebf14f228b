"""Hand-built cases of ngsid_hp_runs (include/ngsid_hp.h): centre, one forward read, the alignment columns WRITTEN BY HAND ('=' 'X' 'I' read only 'D' centre only), the
listed runs and the bucket each collects (-1: the read adds nothing), derived by hand from the definition.  Test infrastructure - never imported by the product.

A case is a core between two fixed flanks of 40 bases without a repeated letter (long enough for the strand rule at k = 13, w = 20, so the same cases run through the
library).  LEFT ends in T and RIGHT begins with G; the cores bring their own flank letters."""
import numpy as np

LEFT = "ACGTACTGATCGATGCTAGCATCGTACGATCTGACTGCAT"
RIGHT = "GCATGTCAGTCTAGCATGCGATCATGCTAGTCGTACGTCA"
NL = len(LEFT)
OPS = {"=": 0, "X": 1, "I": 2, "D": 3}


def ops_array(s):
    return np.array([OPS[c] for c in s], dtype=np.uint8)


def _case(name, core_c, core_r, core_ops, runs, read_left=LEFT, ops_left="=" * NL, read_right=RIGHT, ops_right="=" * len(RIGHT), clip=False):
    """runs: {position in the core: bucket}"""
    starts = sorted(runs)
    return dict(name=name, centre=LEFT + core_c + RIGHT, read=read_left + core_r + read_right, ops=ops_left + core_ops + ops_right,
                starts=[NL + a for a in starts], buckets=[runs[a] for a in starts], clip=clip)


def _sub(s, at):
    """s with the letters at the positions `at` replaced by another letter"""
    s = list(s)
    for i in at: s[i] = "ACGT"[("ACGT".index(s[i]) + 2) % 4]
    return "".join(s)


HAND = [
    # the run AAA of the centre between its flanks C and G (positions 1-3 of the core)
    _case("equal", "CAAAG", "CAAAG", "=====", {1: 3}),
    _case("read_one_longer", "CAAAG", "CAAAAG", "=I====", {1: 4}),                    # qa = 0, qb = 5
    _case("read_one_longer_gap_at_the_end", "CAAAG", "CAAAAG", "====I=", {1: 4}),    # the same bases, the gap elsewhere in the run: the same bucket
    _case("read_one_shorter", "CAAAG", "CAAG", "=D===", {1: 2}),
    _case("read_has_no_base_of_the_run", "CAG", "CG", "=D=", {1: 0}),                 # l = 0
    _case("sixteen_in_the_read", "CAAAG", "C" + "A" * 16 + "G", "=" + "I" * 13 + "====", {1: 15}),
    # a G the centre lacks is not one more A: truth AAAGT, centre AAAT
    _case("foreign_letter_before_the_right_flank", "CAAAT", "CAAAGT", "====I=", {1: 16}),
    _case("foreign_letter_behind_the_left_flank", "CAAAG", "CTAAAG", "=I====", {1: 16}),
    _case("N_inside", "CAAAG", "CANAG", "==X==", {1: 16}),
    _case("left_flank_mismatch", "CAAAG", "GAAAG", "X====", {1: 16}),
    _case("right_flank_deleted", "GAAAC", "GAAA", "====D", {1: 16}),
    # two runs and the run of one base between them: AA (1-2), G (3), TTT (4-6).  Where the aligner puts the inserted A decides what the NEIGHBOUR G sees between its flanks
    _case("neighbours_gap_first", "CAAGTTTC", "CAAAGTTC", "=I====D==", {1: 3, 3: 1, 4: 2}),
    _case("neighbours_gap_last", "CAAGTTTC", "CAAAGTTC", "===I==D==", {1: 3, 3: 16, 4: 2}),
    _case("neighbours_as_the_aligner_walks", "CAAGTTTC", "CAAAGTTC", "===XX===", {1: 16, 3: 16, 4: 16}),     # two mismatches cost what the two gaps cost, and the diagonal wins: no flank left
    _case("run_of_N_in_the_centre", "CNNNG", "CNNNG", "=XXX=", {1: -1}),
    # span edges: the read begins exactly on the left flank / on the first base of the run; ends exactly on the right flank
    _case("span_begins_on_the_flank", "CAAAG", "CAAAG", "=====", {1: 3}, read_left="", ops_left="D" * NL),
    _case("span_begins_on_the_run", "CAAAG", "AAAG", "D====", {1: -1}, read_left="", ops_left="D" * NL),
    _case("span_ends_on_the_flank", "CAAAG", "CAAAG", "=====", {1: 3}, read_right="", ops_right="D" * len(RIGHT)),
    # clip = 1: the counted columns begin with the first run of 15 '='.  Mismatches at 5, 15, 25 and 39 of the left flank: that run begins on the flank C ...
    _case("clip_span_begins_on_the_flank", "CAAAG", "CAAAG", "=====", {1: 3}, read_left=_sub(LEFT, (5, 15, 25, 39)),
          ops_left="".join("X" if i in (5, 15, 25, 39) else "=" for i in range(NL)), clip=True),
    # ... and with the flank itself a mismatch it begins on the run: not spanned under clip, a spanned read without a length otherwise
    _case("clip_flank_mismatch", "CAAAG", "GAAAG", "X====", {1: -1}, read_left=_sub(LEFT, (5, 15, 25)),
          ops_left="".join("X" if i in (5, 15, 25) else "=" for i in range(NL)), clip=True),
    _case("noclip_flank_mismatch", "CAAAG", "GAAAG", "X====", {1: 16}, read_left=_sub(LEFT, (5, 15, 25)),
          ops_left="".join("X" if i in (5, 15, 25) else "=" for i in range(NL))),
    # the first and the last run of a centre are never counted
    dict(name="first_and_last_run", centre=LEFT + "CAAAG" + RIGHT, read=LEFT + "CAAAG" + RIGHT, ops="=" * (NL + 5 + len(RIGHT)),
         starts=[0, NL + 1, NL + 5 + len(RIGHT) - 1], buckets=[-1, 3, -1], clip=False),
]


def check_ops(case):
    """the hand-written columns fit the two sequences: lengths, and '=' exactly where both letters are equal letters of ACGT"""
    c, r, ops = case["centre"], case["read"], case["ops"]
    qi = ti = 0
    for o in ops:
        if o in "=X":
            same = c[ti] == r[qi] and c[ti] in "ACGT"
            assert same == (o == "="), (case["name"], qi, ti)
            qi += 1; ti += 1
        elif o == "I": qi += 1
        else: ti += 1
    assert qi == len(r) and ti == len(c), case["name"]


def with_runs(seq, runs):
    """seq with runs[(position, letter, length)] written over it (the runs lie inside seq and apart); a neighbour that carries the run's letter gets another one, so
    the run has exactly that length"""
    s = list(seq)
    for p, letter, n in runs:
        s[p:p + n] = letter * n
        for x, y in ((p - 1, p - 2), (p + n, p + n + 1)):
            if s[x] == letter: s[x] = next(c for c in "ACGT" if c != letter and c != s[y])
    return "".join(s)


def no_repeat(rng, n, first_not=None):
    """n random letters, no two neighbours equal"""
    out = []; prev = first_not
    for _ in range(n):
        c = "ACGT"[int(rng.integers(4))]
        while c == prev: c = "ACGT"[int(rng.integers(4))]
        out.append(c); prev = c
    return "".join(out)


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def bias_reads(rs, rng, p_short, min_len=4):
    """a read set with every run of at least min_len bases of every read shortened by one with probability p_short (the qualities follow): the length-biased homopolymer
    error the plain read model lacks -> a host ReadSet"""
    from ngspeciesid_amd._capi import ReadSet
    seqs, quals = [], []
    for i in range(rs.n):
        a, b = int(rs.off[i]), int(rs.off[i + 1]); s = rs.seq[a:b]; q = rs.qual[a:b]
        starts = np.concatenate(([0], np.nonzero(s[1:] != s[:-1])[0] + 1, [len(s)])) if len(s) else np.zeros(1, dtype=np.int64)
        keep = np.ones(len(s), dtype=bool)
        for x, y in zip(starts[:-1], starts[1:]):
            if y - x >= min_len and rng.random() < p_short: keep[x] = False
        seqs.append(s[keep]); quals.append(q[keep])
    off = np.zeros(rs.n + 1, dtype=np.uint64); off[1:] = np.cumsum([len(x) for x in seqs])
    return ReadSet(np.concatenate(seqs), np.concatenate(quals), off)
