"""The definition of include/ngsid_chimera.h restated in numpy: what Api.chimera_model must return, field for field and profile for profile.

The DP runs row by row (one row per query prefix, one entry per parent prefix); the dependency inside a row - a cell on the cell to its left - is resolved with
minimum.accumulate(t - j) + j.  The reduction is a plain loop over the pairs of a query, vectorised over the position i only."""
import numpy as np

NFIELD = 7


def _bytes(s):
    return np.frombuffer(s.encode(), dtype=np.uint8) if isinstance(s, str) else np.asarray(s, dtype=np.uint8)


def forward_profile(q, p):
    """F[i] = min over j of ed(q[0:i], p[0:j]), i = 0 .. len(q)"""
    q, p = _bytes(q), _bytes(p)
    n, m = len(q), len(p)
    j = np.arange(m + 1, dtype=np.int64)
    row = j.copy()                                  # ed("", p[0:j]) = j
    F = np.zeros(n + 1, dtype=np.int64)
    t = np.empty(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        t[0] = i
        if m:
            np.minimum(row[:-1] + (p != q[i - 1]), row[1:] + 1, out=t[1:])
        row = np.minimum.accumulate(t - j) + j      # cell j also reaches every cell to its left at one edit per step
        F[i] = row.min()
    return F


def profiles_of(q, p):
    """(F, B) of one pair: B is F of the reversed strings, read backwards"""
    q, p = _bytes(q), _bytes(p)
    return forward_profile(q, p), forward_profile(q[::-1], p[::-1])[::-1].copy()


def reduce_query(Fs, Bs, gids, n):
    """the seven fields of a query from the profiles of its pairs (lists of int64 arrays) and their gids"""
    P = len(Fs)
    out = [-1] * NFIELD
    if P == 0:
        return out
    ends = [int(F[n]) for F in Fs]
    out[1] = min(ends); out[0] = ends.index(out[1])
    best = None
    for a in range(P):
        for b in range(P):
            if gids[a] == gids[b]:
                continue
            s = Fs[a] + Bs[b]
            c = int(s.min()); i = int(np.argmin(s))               # the first (smallest) i
            if best is None or (c, i) < (best[0], best[1]):       # pairs arrive in lexicographic order: a tie keeps the earlier pair
                best = (c, i, a, b)
    if best is not None:
        c, i, a, b = best
        hi = int(np.nonzero(Fs[a] + Bs[b] == c)[0][-1])
        out[2:] = [c, a, b, i, hi]
    return out


def chimera_model(queries, parents, pair_off, pair_parent, pair_gid=None, cache=None):
    """-> (fields [n, 7] int32, profiles uint16, prof_off [n_pairs + 1] uint64) as Api.chimera_model(..., profiles=True) returns them.
    queries / parents: lists of strings.  cache: a dict that keeps the profiles of (query, parent) string pairs between calls."""
    pair_off = np.asarray(pair_off).astype(np.int64); pair_parent = np.asarray(pair_parent).astype(np.int64)
    gid = pair_parent if pair_gid is None else np.asarray(pair_gid).astype(np.int64)
    nq = len(queries)
    fields = np.full((nq, NFIELD), -1, dtype=np.int32)
    prof_off = np.zeros(len(pair_parent) + 1, dtype=np.uint64)
    blocks = []
    cache = {} if cache is None else cache
    for qi, q in enumerate(queries):
        n = len(q)
        Fs, Bs = [], []
        for k in range(int(pair_off[qi]), int(pair_off[qi + 1])):
            key = (q, parents[int(pair_parent[k])])
            if key not in cache:
                cache[key] = profiles_of(*key)
            F, B = cache[key]
            Fs.append(F); Bs.append(B)
            blocks.append(F); blocks.append(B)
            prof_off[k + 1] = prof_off[k] + np.uint64(2 * (n + 1))
        fields[qi] = reduce_query(Fs, Bs, [int(g) for g in gid[int(pair_off[qi]):int(pair_off[qi + 1])]], n)
    prof = np.concatenate(blocks).astype(np.uint16) if blocks else np.zeros(0, dtype=np.uint16)
    return fields, prof, prof_off
