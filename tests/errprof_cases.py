"""Hand-built cases of ngsid_error_profile (include/ngsid_errprof.h): centre, read as it is handed in, its quality string, and the tables WRITTEN OUT BY HAND from the
definition.  Test infrastructure - never imported by the product.

A case is a core between the two flanks of tests/hp_cases.py (40 bases each, no two neighbours equal, long enough for the strand rule at k = 13, w = 20, so the same cases
run through the library).  The cores begin with C (LEFT ends in T) and end with T or A (RIGHT begins with G): every centre run outside the core has length 1.  Every core
has ONE minimum-cost alignment, or one the aligner's tie-break fixes inside a run of equal letters, where the tables do not depend on it."""
import numpy as np
from hp_cases import LEFT, RIGHT, revcomp, _sub

NCOUNT, NQ = 96, 94
PAIR, INS_LETTER, CEN_OTHER, READS, INS_LEN, DEL_LEN, HPCTX = 0, 24, 29, 30, 32, 48, 64
A, C, G, T, OTHER, DEL = 0, 1, 2, 3, 4, 5
HP_EQ, HP_X, HP_D, HP_INS = 0, 1, 2, 3
Q40 = "I"                                                                    # the quality byte of every base a case says nothing about: 73 - 33 = 40


def _letters(s):
    """{PAIR cell of an '=' column: count} of the centre letters s"""
    return {PAIR + "ACGT".index(c) * 7: s.count(c) for c in "ACGT" if s.count(c)}


def _table(eq, eq_runs, extra):
    """counts [96]: the '=' columns of the centre letters eq, which sit in centre runs eq_runs = {run length: columns}, and the cells of extra"""
    t = np.zeros(NCOUNT, dtype=np.uint64)
    for k, v in _letters(eq).items(): t[k] += np.uint64(v)
    assert sum(eq_runs.values()) == len(eq)
    for r, v in eq_runs.items(): t[HPCTX + (min(r, 8) - 1) * 4 + HP_EQ] += np.uint64(v)
    for k, v in extra.items(): t[k] += np.uint64(v)
    t[READS] += np.uint64(1)
    return t


def _qtable(cells):
    q = np.zeros((NQ, 3), dtype=np.uint64)
    for (qq, k), v in cells.items(): q[qq, k] += np.uint64(v)
    return q


def _case(name, core_c, core_r, qual_core=None, strand=0, counts=None, qtab=None, counts_clip=None, qtab_clip=None, read_left=LEFT, tail="", ramp=False):
    centre = LEFT + core_c + RIGHT
    read = read_left + core_r + RIGHT + tail
    qual = Q40 * len(read_left) + (qual_core or Q40 * len(core_r)) + Q40 * len(RIGHT) + "!" * len(tail)
    if ramp: qual = "".join(chr(33 + i) for i in range(len(read)))                # byte i of the read AS HANDED IN reports quality i
    if strand == 1: read = revcomp(read)                                        # (the qualities stay: they belong to the read as it is handed in)
    assert len(qual) == len(read)
    return dict(name=name, centre=centre, read=read, qual=qual, strand=strand, counts={False: counts, True: counts if counts_clip is None else counts_clip},
                qtab={False: qtab, True: qtab if qtab_clip is None else qtab_clip})


FL = LEFT + RIGHT                                                             # the 80 flank letters, every one a run of 1
_CLIP_AT = (5, 15, 25, 39)                                                    # mismatches of the clip case: no run of 15 '=' in front of the core

HAND = [
    # A -> G at centre position 41, reported with quality 10 ('+')
    _case("substitution", "CAT", "CGT", qual_core=Q40 + "+" + Q40,
          counts=_table(FL + "CT", {1: 82}, {PAIR + A * 6 + G: 1, HPCTX + 0 * 4 + HP_X: 1}), qtab=_qtable({(40, 0): 82, (10, 1): 1})),
    # a G the centre lacks between A and T, quality 5 ('&'): behind a run of 1
    _case("insertion_of_1", "CAT", "CAGT", qual_core=Q40 * 2 + "&" + Q40,
          counts=_table(FL + "CAT", {1: 83}, {INS_LETTER + G: 1, INS_LEN + 0: 1, HPCTX + 0 * 4 + HP_INS: 1}), qtab=_qtable({(40, 0): 83, (5, 2): 1})),
    # two of the three A deleted: one 'D' run of 2, wherever in the run the aligner puts it
    _case("deletion_of_2_in_a_run_of_3", "CAAAT", "CAT",
          counts=_table(FL + "CAT", {1: 82, 3: 1}, {PAIR + A * 6 + DEL: 2, DEL_LEN + 1: 1, HPCTX + 2 * 4 + HP_D: 2}), qtab=_qtable({(40, 0): 83})),
    # an N in the read: a mismatch whose read letter is outside ACGT, quality 2 ('#')
    _case("N_in_the_read", "CAT", "CNT", qual_core=Q40 + "#" + Q40,
          counts=_table(FL + "CT", {1: 82}, {PAIR + A * 6 + OTHER: 1, HPCTX + 0 * 4 + HP_X: 1}), qtab=_qtable({(40, 0): 82, (2, 1): 1})),
    # an N in the centre: a mismatch without a PAIR row and without a run
    _case("N_in_the_centre", "CNT", "CAT", qual_core=Q40 + "5" + Q40,
          counts=_table(FL + "CT", {1: 82}, {CEN_OTHER: 1}), qtab=_qtable({(40, 0): 82, (20, 1): 1})),
    # the reverse complement of LEFT C G T A RIGHT (84 letters) with byte i reporting quality i: the mismatch sits at oriented position 41 = byte 83 - 41 = 42 of the read as
    # it is handed in (a table built from un-reversed qualities has it at 41)
    _case("minus_strand_quality_ramp", "CATA", "CGTA", strand=1, ramp=True,
          counts=_table(FL + "CTA", {1: 83}, {PAIR + A * 6 + G: 1, HPCTX + 0 * 4 + HP_X: 1}), qtab=_qtable(dict([((q, 0), 1) for q in range(84) if q != 42] + [((42, 1), 1)]))),
    # two read letters behind the centre's last base: an 'I' run behind the last counted column, not counted (nor are its qualities, 0 = '!')
    _case("insertion_behind_the_last_counted_column", "CAT", "CAT", tail="TT",
          counts=_table(FL + "CAT", {1: 83}, {}), qtab=_qtable({(40, 0): 83})),
    # mismatches at 5, 15, 25 and 39 of the left flank: with clip the counted columns begin at the core (no run of 15 '=' in front of it), without it at column 0
    _case("clip", "CAT", "CAT", read_left=_sub(LEFT, _CLIP_AT),
          counts=_table("".join(c for i, c in enumerate(LEFT) if i not in _CLIP_AT) + "CAT" + RIGHT, {1: 79},
                        dict([(HPCTX + 0 * 4 + HP_X, 4)] + [(PAIR + "ACGT".index(LEFT[i]) * 6 + ("ACGT".index(LEFT[i]) + 2) % 4, sum(LEFT[j] == LEFT[i] for j in _CLIP_AT)) for i in _CLIP_AT])),
          qtab=_qtable({(40, 0): 79, (40, 1): 4}),
          counts_clip=_table("CAT" + RIGHT, {1: 43}, {}), qtab_clip=_qtable({(40, 0): 43})),
]


def hand_sets():
    """-> (centres, reads, quals, grp_off, strand): every case a group of its own with one read"""
    return ([c["centre"] for c in HAND], [c["read"] for c in HAND], [c["qual"] for c in HAND], np.arange(len(HAND) + 1, dtype=np.uint64), [c["strand"] for c in HAND])


def hand_expected(clip):
    """-> (counts [n, 2, 96], qtab [n, 2, 94, 3]) of hand_sets()"""
    counts = np.zeros((len(HAND), 2, NCOUNT), dtype=np.uint64); qtab = np.zeros((len(HAND), 2, NQ, 3), dtype=np.uint64)
    for g, c in enumerate(HAND):
        counts[g, c["strand"]] = c["counts"][clip]; qtab[g, c["strand"]] = c["qtab"][clip]
    return counts, qtab
