"""Case builders for the front-end reference tests (test_frontend_reference_cpu.py, test_gpu_frontend_reference.py): read sets for ngsid_score_reads and
ngsid_hpc_minimizers at the smallest shapes at which the kernels can go wrong, all seeded.  A case is one call: a dict with the call's arguments, its reads
as Python strings, and what the test needs to know about single reads.  The expected results come from tests/frontend_reference.py and are computed once per
case (score_expected / minimizer_expected), whichever test asks first.

Why these shapes (csrc/ngsid_api.hip k_score_reads, csrc/k_minimizers.hip):
  scores      one lane per read, 64 reads per wave, bases and qualities pass through LDS in 64-byte slices, the leaving quality comes from a 128-byte ring
              (k <= 64: k = 64 reads it exactly one slice back); a slice is loaded as dwords where four bytes remain, else byte by byte; the quality histogram
              has 16-bit counters up to 65 535 bases per read and 32-bit ones beyond.
  minimizers  one wave per read, staged as dwords from the first aligned address (head / tail bytes apart); four layouts: registers (W = w - k + 1 <= 16 by
              default, <= 32 on request; 64 - (W - 1) windows per 64-lane chunk), stored, lean, long; one-word codes to k = 21 (63 bits), two words above.
"""
from functools import lru_cache
import numpy as np
import frontend_reference as fr

THR = 7.0
SCORE_KS = (1, 2, 13, 31, 63, 64)
KW_PAIRS = ((1, 1), (1, 255), (3, 3), (4, 19), (5, 5), (13, 20), (20, 35), (21, 21), (21, 36), (21, 37), (12, 43), (16, 47), (16, 48), (13, 76), (13, 77),
            (22, 22), (22, 40), (25, 30), (32, 32), (32, 40), (32, 255),
            (7, 8))            # (the only pair with a window of two k-mers: one doubling step less than any other)


# ---------------------------------------------------------------------------------------------- strings
def rand_seq(rng, n, letters="ACGT"):
    return "".join(letters[i] for i in rng.integers(0, len(letters), n))


def rand_qual(rng, n, lo=33, hi=33 + 59):
    """quality characters with codes lo .. hi (default Q0 .. Q59)"""
    return "".join(chr(c) for c in rng.integers(lo, hi + 1, n))


def no_hp(rng, n, letters="ACGTN", prev=""):
    """n letters, no two neighbours equal (and the first differs from `prev`): the HPC string is the string itself"""
    out = []
    for _ in range(n):
        c = prev
        while c == prev:
            c = letters[int(rng.integers(0, len(letters)))]
        out.append(c); prev = c
    return "".join(out)


def with_repeats(rng, n, letters="ACGTN"):
    """n letters in runs: 30 % of the runs are homopolymers of 2 .. 6 bases"""
    out, prev = "", ""
    while len(out) < n:
        c = no_hp(rng, 1, letters, prev)
        out += c * (int(rng.integers(2, 7)) if rng.random() < 0.3 else 1); prev = c
    return out[:n]


# ---------------------------------------------------------------------------------------------- scores
def _score_case(name, k, seqs, quals, tags=None, exact=True):
    assert all(len(s) == len(q) for s, q in zip(seqs, quals))
    return dict(name="k%d-%s" % (k, name), k=k, thr=THR, seqs=list(seqs), quals=list(quals), tags=list(tags or [None] * len(seqs)), exact=exact)


@lru_cache(maxsize=None)
def score_cases():
    """tags: 'on' = built to sit exactly on the threshold, 'above' / 'below' = its two neighbours"""
    cases = []
    for k in SCORE_KS:
        rng = np.random.default_rng(1000 + k)
        rd = lambda n: (rand_seq(rng, n), rand_qual(rng, n))
        # every length at which a path changes: 2k (the drop rule), the 64-byte slices, the 128-byte ring, many slices
        lens = sorted(set([2 * k - 1, 2 * k, 2 * k + 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 700, 4000]))
        cases.append(_score_case("lengths", k, *zip(*[rd(n) for n in lens])))
        # batch sizes around one wave of 64 reads
        for n in (1, 63, 64, 65, 129):
            cases.append(_score_case("batch%d" % n, k, *zip(*[rd(int(rng.integers(max(2 * k - 1, 1), 2 * k + 70))) for _ in range(n)])))
        # one wave whose loop count is set by one lane: empty, 1 base, 2k - 1, HPC length < k at length >= 2k, and 4 000 bases
        hp = "A" * (2 * k) + "C" * (k > 2)                                     # (k = 1: no read has an HPC length below k)
        mixed = [("", ""), rd(1), rd(2 * k - 1), (hp, rand_qual(rng, len(hp))), rd(4000)]
        cases.append(_score_case("mixed-wave", k, *zip(*mixed)))
        # read starts = 0..3 mod 4 x lengths = 0..3 mod 4: 1-, 2- and 3-base reads in front move the start
        reads, at = [], 0
        for start in range(4):
            for lm in range(4):
                pad = (start - at) % 4
                if pad: reads.append(rd(pad)); at += pad
                n = 4 * ((2 * k + 3) // 4) + 64 + lm
                reads.append(rd(n)); at += n
        cases.append(_score_case("offsets", k, *zip(*reads)))
        # qualities: the clamp ('!': P 0.79433, RAW 1.0 - the error rate is exactly 1), the first character above it, the last printable one, all 94 printable
        # characters (the longest ordered sum), random
        n = 2 * k + 172
        allq = "".join(chr(33 + i % 94) for i in range(n))
        qs = ["!" * n, '"' * n, "~" * n, allq, rand_qual(rng, n)]
        cases.append(_score_case("qualities", k, [rand_seq(rng, n) for _ in qs], qs))
        # the threshold: 400 x '(' has a phred of 7.0 up to the rounding of log(); one better / one worse character moves it by 2e-3
        s = rand_seq(rng, 400)
        cases.append(_score_case("threshold", k, [s, s, s], ["(" * 400, "(" * 399 + ")", "(" * 399 + "'"], tags=["on", "above", "below"]))
    # histogram counters: 65 535 equal characters fill the 16-bit counter exactly; a set with a read of 65 536 runs the 32-bit instance (float replay only)
    rng = np.random.default_rng(77)
    for n in (65535, 65536):
        seqs = [rand_seq(rng, 150), rand_seq(rng, n), rand_seq(rng, 70)]
        quals = [rand_qual(rng, 150), "5" * n, rand_qual(rng, 70)]
        cases.append(_score_case("histogram%d" % n, 13, seqs, quals, exact=False))
    return tuple(cases)


@lru_cache(maxsize=None)
def score_expected(i):
    c = score_cases()[i]
    return fr.scores_ref(c["seqs"], c["quals"], c["k"], c["thr"])


# ---------------------------------------------------------------------------------------------- minimizers
def tie_read():
    """the run-quality tie that shows in the result: m runs of two bases with the qualities ' ' then '!' (equal P: the FIRST, ' ', is the run's quality), and
    j one-base runs with '!'.  First on ties: the histogram is {' ': m, '!': j} and the sum fl(m P) + fl(j P); last on ties: {'!': m + j} and fl((m + j) P).
    (m, j) = the first pair for which the two differ as doubles after the division (checked here on the table value alone)."""
    p = fr.P[33]
    assert fr.P[32] == p
    for m in range(1, 40):
        for j in range(1, 40):
            if (float(m) * p + float(j) * p) / float(m + j) != (float(m + j) * p) / float(m + j):
                seq = "".join("ACGT"[i % 4] * (2 if i < m else 1) for i in range(m + j))
                return seq, " !" * m + "!" * j
    raise AssertionError("no such pair")


def _wide_reads(rng, k, w):
    """k > 21: three reads whose first k-mer is a minimizer (it starts with the only A or C of the read): A and B agree in the last 21 letters (the low code
    word) and differ before, A and C agree before and differ in the last letter"""
    x = no_hp(rng, k - 1, "GNT")
    last = [c for c in "GNT" if c not in x[-2:]][0]
    heads = ["A" + x, "C" + x, "A" + x[:-1] + last]
    return [h + no_hp(rng, w + 5, "GNT", h[-1]) for h in heads]


def _mz_case(name, k, w, seqs, quals, bad=None):
    assert quals is None or all(len(s) == len(q) for s, q in zip(seqs, quals))
    return dict(name="k%d-w%d-%s" % (k, w, name), k=k, w=w, seqs=list(seqs), quals=None if quals is None else list(quals), bad=bad)


@lru_cache(maxsize=None)
def minimizer_cases():
    """per (k, w): 'main' (with qualities), 'noqual' (the same reads without), 'alphabet' and, for k > 1, 'alphabet-short' (bad = the reads that hold a foreign base), k > 21: 'single'"""
    cases = []
    for k, w in KW_PAIRS:
        rng = np.random.default_rng(5000 + 300 * k + w)
        W = w - k + 1
        lens = [1, 2, 3, k - 1, k, k + 1, k + 2, w - 1, w, w + 1, 2 * w, 63, 64, 65, 64 + k - 1, 64 + w - 1, 128 + w - 1, 750]
        if W <= 32:                                                                # the chunk seams of the register layout: 64 - (W - 1) windows per chunk
            lens += [(64 - (W - 1)) * m + w - 1 + d for m in (1, 2) for d in (-1, 0, 1)]
        seqs = []
        for n in sorted(set(x for x in lens if x >= 0)):
            seqs += [no_hp(rng, n), with_repeats(rng, n)]
        quals = [rand_qual(rng, len(s)) for s in seqs]
        add = lambda s, q=None: (seqs.append(s), quals.append(rand_qual(rng, len(s)) if q is None else q))
        add("AC" * 200); add("A" * 300); add("ACGTN" * 60); add("N" * 5 + "ACGT" * 30)
        add("")                                                                    # an empty read in the middle
        # a run of 200 equal bases from base 40 on, across four 64-lane chunks: its best quality ('Z') sits in the last chunk; once alone, once with an equal one earlier
        s = no_hp(rng, 40, "ACT") + "G" * 200 + no_hp(rng, 60, "ACGT", "G")
        for first in (230, 100):
            q = list(rand_qual(rng, 300, 38, 63)); q[230] = "Z"; q[first] = "Z"
            add(s, "".join(q))
        add(no_hp(rng, 50, "ACG") + "T" * 10)                                     # a run ends the read
        s = with_repeats(rng, 120); add(s, rand_qual(rng, 120, 20, 33))           # qualities up to '!': every character of a run ties, the first is its quality
        add(*tie_read())
        # 1- and 2-base reads whose start is 1, 2, 3 mod 4 (fewer bytes than the staging loop's unaligned head)
        at = sum(len(x) for x in seqs)
        for start in (1, 2, 3):
            for n in (1, 2):
                pad = (start - at) % 4 + 4
                add(no_hp(rng, pad)); add(no_hp(rng, n)); at += pad + n
        if k > 21:
            s = no_hp(rng, 100)
            for x in (s, s, s): add(x)                                             # equal ranks across reads
            for x in _wide_reads(rng, k, w): add(x)
        cases.append(_mz_case("main", k, w, seqs, quals))
        cases.append(_mz_case("noqual", k, w, seqs, None))
        if k > 21:
            s = no_hp(rng, k); cases.append(_mz_case("single", k, w, [s], [rand_qual(rng, k)]))       # the whole call emits one minimizer
        # a lower-case base in read 3 and an X in read 7 of 9
        bad = [no_hp(rng, w + 30) for _ in range(9)]
        bad[3] = bad[3][:20] + bad[3][20].lower() + bad[3][21:]
        bad[7] = bad[7][:11] + "X" + bad[7][12:]
        cases.append(_mz_case("alphabet", k, w, bad, [rand_qual(rng, len(s)) for s in bad], bad=[3, 7]))
        if k > 1:
            # the same for a read too short to have a k-mer (HPC length k - 1): the encoder meets its letters all the same
            short = [no_hp(rng, w + 30) for _ in range(4)] + ["X" + no_hp(rng, k - 2)] + [no_hp(rng, w + 30) for _ in range(4)]
            cases.append(_mz_case("alphabet-short", k, w, short, [rand_qual(rng, len(s)) for s in short], bad=[4]))
    return tuple(cases)


@lru_cache(maxsize=None)
def minimizer_expected(i):
    """the reference's (mz_off, codes, pos, hpc_len, hpc_err) of case i; for an alphabet case the AlphabetError itself"""
    c = minimizer_cases()[i]
    try:
        return fr.call_ref(c["seqs"], c["quals"], c["k"], c["w"])
    except fr.AlphabetError as e:
        return e


def read_set(case):
    from ngspeciesid_amd._capi import ReadSet
    return ReadSet.from_strings(case["seqs"], case["quals"])


def describe_read(case, r):
    """what a failure message says about read r of a case: length and start offset mod 4"""
    at = sum(len(s) for s in case["seqs"][:r])
    return "read %d (length %d, start %d mod 4)" % (r, len(case["seqs"][r]), at % 4)


def first_difference(case, got, exp, names, per_read=()):
    """None when every array of `got` equals its twin in `exp` (NaN == NaN), else a line naming the case and the first entry that differs"""
    for nm, g, e in zip(names, got, exp):
        g, e = np.asarray(g), np.asarray(e)
        if g.shape != e.shape:
            return "%s: %s has %d entries, expected %d" % (case["name"], nm, g.size, e.size)
        ne = g != e
        if g.dtype.kind == "f": ne &= ~(np.isnan(g) & np.isnan(e))
        if ne.any():
            i = int(np.argmax(ne))
            return "%s: %s[%d] = %r, expected %r%s" % (case["name"], nm, i, g[i].item(), e[i].item(), " - " + describe_read(case, i) if nm in per_read else "")
    return None
