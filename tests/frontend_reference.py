"""A plain reference of the front end - ngsid_score_reads (f1) and ngsid_hpc_minimizers (a1-a3) of include/ngsid.h - in Python
strings, floats and Fractions, one read at a time.  Written from the header's (f1) / (a1-a3) comments and DESIGN.md; it shares no code
with oracle/ or the library, and is the anchor that oracle and kernels are both compared with.

Tables.  P[c] = min(10 ** (-(c - 33) / 10.0), 0.79433) and RAW[c] = 10 ** (-(c - 33) / 10.0) for the quality character codes c = 0..127.

Score (f1).  With q the qualities of a read of L bases, N = L - k + 1:  cur = product of (1 - P[q[i]]) over the first k characters, formed left to
right from 1.0; sum = cur; then for i = k .. L-1: cur *= (1 - P[q[i]]) / (1 - P[q[i-k]]); sum += cur.  score = (1 - (N - sum) / N) * N.  Python floats
are IEEE doubles, so this IS the sequence of operations the library promises to replay.  err = (sum over the quality characters that occur, in
ascending character code, of count * RAW[c], starting from the first term) / L.  keep = 0 when L < 2k, when the HPC length < k (both: score = err =
0.0, nothing is computed), or when 10 * -log(err, 10) <= threshold; log(x, 10) = log(x) / log(10).

HPC (a1, a3).  One letter per run of equal bases.  The quality of a run is the character of the run with the LOWEST P, the first such character on
ties (every character up to '!' has the same P).  HPC error rate = (sum over the run qualities that occur, ascending character code, of
count * P[c]) / HPC length; NaN without qualities or for an empty read.

Minimizers (a2).  h = HPC string, n = len(h), nk = n - k + 1, W = w - k + 1.  A read with n < k has none.  The k-mers are h[i:i+k] for
i < max(nk, W): slices that run past the end are proper prefixes, or empty, and sort BEFORE their extensions (plain string order, which
is byte order: A < C < G < N < T).  Window s = k-mers s .. s+W-1, for s < max(nk - W + 1, 1); its minimizer is the LEFTMOST minimum; a minimizer is
emitted when its position differs from the one before it.

Codes.  k <= 21: 3 bits per letter (A 1, C 2, G 3, N 4, T 5), first letter most significant, zeros past the end of a truncated k-mer.
k > 21: the dense rank of the k-mer string among all strings emitted by the call (equal strings equal rank).
"""
import math
from fractions import Fraction
from itertools import groupby
import numpy as np

P = [min(10 ** (-(c - 33) / 10.0), 0.79433) for c in range(128)]
RAW = [10 ** (-(c - 33) / 10.0) for c in range(128)]
LETTER = {"A": 1, "C": 2, "G": 3, "N": 4, "T": 5}


class AlphabetError(ValueError):
    """a base outside ACGTN; .reads = the reads of the call that hold one (the library names any ONE of them)"""

    def __init__(self, reads):
        super().__init__("reads %s: base outside ACGTN" % reads)
        self.reads = list(reads)


def _q(qual):
    c = [ord(ch) for ch in qual]
    assert all(x < 128 for x in c)
    return c


def hpc_string(seq):
    return "".join(ch for ch, _ in groupby(seq))


def ordered_sum(chars, table):
    """sum over the characters that occur, ascending code, of count x table[c]; the first term starts the sum"""
    total = None
    for c in sorted(set(chars)):
        term = float(chars.count(c)) * table[c]
        total = term if total is None else total + term
    return total


def phred_of(err):
    return 10 * -math.log(err, 10)


def score_ref(seq, qual, k, thr):
    """-> (score, err, keep) of one read"""
    L = len(seq)
    if L < 2 * k or len(hpc_string(seq)) < k:
        return 0.0, 0.0, 0
    q = _q(qual)
    cur = 1.0
    for i in range(k):
        cur = cur * (1.0 - P[q[i]])
    total = cur
    for i in range(k, L):
        cur *= (1.0 - P[q[i]]) / (1.0 - P[q[i - k]])
        total += cur
    N = float(L - k + 1)
    score = (1.0 - (N - total) / N) * N
    err = ordered_sum(q, RAW) / float(L)
    return score, err, (0 if phred_of(err) <= thr else 1)


def score_exact(qual, k):
    """the sum over all windows of k characters of the product of (1 - P[c]), in exact arithmetic on the table's doubles (no recurrence)"""
    f = [1 - Fraction(P[c]) for c in _q(qual)]
    D = max(x.denominator for x in f)                  # doubles: every denominator is a power of two, so D is their common multiple
    m = [int(x * D) for x in f]                        # f[i] = m[i] / D exactly
    assert all(Fraction(a, D) == x for a, x in zip(m, f))
    return Fraction(sum(math.prod(m[i:i + k]) for i in range(len(m) - k + 1)), D ** k)


def hpc_ref(seq, qual=None):
    """-> (HPC string, run qualities (str) or None, HPC error rate)"""
    h, hq, i = [], [], 0
    for ch, run in groupby(seq):
        n = len(list(run))
        h.append(ch)
        if qual is not None:
            hq.append(min(qual[i:i + n], key=lambda c: P[ord(c)]))        # min() keeps the first of equal keys
        i += n
    h = "".join(h)
    if qual is None or not h:
        return h, (None if qual is None else ""), float("nan")
    hq = "".join(hq)
    return h, hq, ordered_sum(_q(hq), P) / float(len(h))


def minimizers_ref(h, k, w):
    """-> [(k-mer string, position)] of one HPC string with len(h) >= k"""
    n = len(h)
    nk, W = n - k + 1, w - k + 1
    kmers = [h[i:i + k] for i in range(max(nk, W))]
    out, prev = [], -1
    for s in range(max(nk - W + 1, 1)):
        win = kmers[s:s + W]
        p = s + win.index(min(win))                                        # index() = the leftmost
        if p != prev:
            out.append((kmers[p], p)); prev = p
    return out


def code3(kmer, k):
    c = 0
    for t in range(k):
        c = c * 8 + (LETTER[kmer[t]] if t < len(kmer) else 0)
    return c


def codes_ref(kmers, k):
    """codes of ALL the k-mer strings a call emits, in emission order"""
    if k <= 21:
        return [code3(s, k) for s in kmers]
    rank = {s: r for r, s in enumerate(sorted(set(kmers)))}
    return [rank[s] for s in kmers]


def call_ref(seqs, quals, k, w):
    """one ngsid_hpc_minimizers call -> (mz_off uint64[n+1], codes uint64, pos uint32, hpc_len uint32[n], hpc_err float64[n]); AlphabetError when a
    read holds a base outside ACGTN"""
    bad = [i for i, s in enumerate(seqs) if any(ch not in LETTER for ch in s)]
    if bad:
        raise AlphabetError(bad)
    moff, kmers, pos, hl, he = [0], [], [], [], []
    for i, s in enumerate(seqs):
        h, _, e = hpc_ref(s, None if quals is None else quals[i])
        hl.append(len(h)); he.append(e)
        if len(h) >= k:
            for km, p in minimizers_ref(h, k, w):
                kmers.append(km); pos.append(p)
        moff.append(len(pos))
    return (np.array(moff, dtype=np.uint64), np.array(codes_ref(kmers, k), dtype=np.uint64), np.array(pos, dtype=np.uint32),
            np.array(hl, dtype=np.uint32), np.array(he, dtype=np.float64))


def scores_ref(seqs, quals, k, thr):
    """one ngsid_score_reads call -> (score, err, keep uint8, phred) arrays; phred = 10 * -log(err, 10) of the reads that got that far, else NaN"""
    sc, er, kp, ph = [], [], [], []
    for s, q in zip(seqs, quals):
        a, b, c = score_ref(s, q, k, thr)
        sc.append(a); er.append(b); kp.append(c)
        ph.append(phred_of(b) if b > 0.0 else float("nan"))
    return np.array(sc), np.array(er), np.array(kp, dtype=np.uint8), np.array(ph)
