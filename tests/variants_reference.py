"""Independent restatement of include/ngsid_near.h and of the policy of ngspeciesid_amd/variants.py in numpy and plain loops.  Shares no code with either."""
import functools
import numpy as np

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def rc(s):
    return "".join(_COMP[c] for c in reversed(s))


@functools.lru_cache(maxsize=None)
def ed(a, b):
    """unit-cost global edit distance, the full rectangle row by row.  Within a row cur[j] = min(cand[j], cur[j - 1] + 1) unrolls to
    min over k <= j of cand[k] + (j - k), a running minimum of cand[k] - k."""
    n = len(b)
    if len(a) == 0: return n
    if n == 0: return len(a)
    bb = np.frombuffer(b.encode(), dtype=np.uint8)
    ar = np.arange(n + 1, dtype=np.int64)
    prev = ar.copy()
    for i, ch in enumerate(a.encode(), start=1):
        cand = np.empty(n + 1, dtype=np.int64)
        cand[0] = i
        cand[1:] = np.minimum(prev[:-1] + (bb != ch), prev[1:] + 1)
        prev = np.minimum.accumulate(cand - ar) + ar
    return int(prev[n])


def D(a, b, both_strands=True):
    """-> (distance, strand): a tie goes to forward"""
    f = ed(a, b)
    if not both_strands: return f, 0
    r = ed(a, rc(b))
    return (r, 1) if r < f else (f, 0)


def ed_within(queries, targets, q_idx, t_idx, max_dist, both_strands=True):
    """-> (dist int32 [n], strand uint8 [n]): -1 / 0 where the distance exceeds max_dist"""
    dist = np.full(len(q_idx), -1, dtype=np.int32); strand = np.zeros(len(q_idx), dtype=np.uint8)
    for p, (q, t) in enumerate(zip(q_idx, t_idx)):
        d, s = D(queries[int(q)], targets[int(t)], both_strands)
        if d <= max_dist: dist[p], strand[p] = d, s
    return dist, strand


def ed_many(a, bs):
    """ed(a, b) for every b of bs: the same rectangle as ed(), all of them side by side (b padded with a byte that equals nothing; the cell (len a, len b) does not
    depend on the columns behind it) -> int64 [len(bs)]"""
    if not bs: return np.zeros(0, dtype=np.int64)
    lens = np.array([len(b) for b in bs], dtype=np.int64); n = int(lens.max())
    B = np.zeros((len(bs), n), dtype=np.uint8)
    for k, b in enumerate(bs): B[k, :len(b)] = np.frombuffer(b.encode(), dtype=np.uint8)
    ar = np.arange(n + 1, dtype=np.int64)
    prev = np.tile(ar, (len(bs), 1))
    for i, ch in enumerate(a.encode(), start=1):
        cand = np.empty_like(prev)
        cand[:, 0] = i
        cand[:, 1:] = np.minimum(prev[:, :-1] + (B != ch), prev[:, 1:] + 1)
        prev = np.minimum.accumulate(cand - ar, axis=1) + ar
    return prev[np.arange(len(bs)), lens]


def near_pairs(seqs, max_dist, both_strands=True):
    """brute force over all i < j -> [(i, j, dist, strand)] in ascending (i, j) order"""
    out = []
    rcs = [rc(s) for s in seqs]
    for i in range(len(seqs) - 1):
        f = ed_many(seqs[i], seqs[i + 1:])
        r = ed_many(seqs[i], rcs[i + 1:]) if both_strands else None
        for k in range(len(f)):
            d, s = (int(r[k]), 1) if both_strands and r[k] < f[k] else (int(f[k]), 0)
            if d <= max_dist: out.append((i, i + 1 + k, d, s))
    return out


def _frac(identity):
    """'0.97' -> (97, 100) without a float in between"""
    text = str(identity).strip()
    whole, _, frac = text.partition(".")
    return int((whole or "0") + frac), 10 ** len(frac)


def thresholds(lengths, identity, max_dist):
    """threshold of pair (i, j) = min(max_dist, floor((1 - identity) * max(len_i, len_j))) -> a function (i, j) -> int"""
    num, den = _frac(identity)
    def thr(i, j):
        L = max(int(lengths[i]), int(lengths[j]))
        return min(int(max_dist), ((den - num) * L) // den)
    return thr


def cluster(sizes, lengths, seqs, pairs, thr):
    """greedy centroid clustering by abundance, plain loops: pairs = [(i, j, dist, strand)], thr(i, j) -> int.  -> (variant_of [n], centroid [n_variants],
    dist [n], strand [n]): every sequence in (reads desc, length desc, bytes asc, index asc) order joins the earliest centroid within the pair's threshold or founds
    a variant; variants are numbered in founding order"""
    n = len(seqs)
    near = {}
    for i, j, d, s in pairs:
        if d <= thr(i, j):
            near[(i, j)] = (d, s); near[(j, i)] = (d, s)
    order = sorted(range(n), key=lambda x: (-int(sizes[x]), -int(lengths[x]), seqs[x].encode(), x))
    variant_of, dist, strand, cents = [-1] * n, [0] * n, [0] * n, []
    for x in order:
        for v, c in enumerate(cents):
            if (x, c) in near:
                variant_of[x] = v; dist[x], strand[x] = near[(x, c)]
                break
        else:
            variant_of[x] = len(cents); cents.append(x)
    return variant_of, cents, dist, strand
