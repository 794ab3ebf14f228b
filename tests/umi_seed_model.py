"""The seeded neighbour search of csrc/k_umi.hip on Python ints, step for step - test infrastructure, not a test: the letter planes, the seed keys, the sorted
index, the ranges of a query's substrings (entries of a smaller sequence index only), the first-witness rule, the 64-bit Myers column with the tracked diagonal and
the short path over the set ordered by length.  Every verification is recorded, so a test can tell that each pair went through the column exactly once."""
import bisect

M64 = (1 << 64) - 1
NOKEY = (15 << 48) | 0xffffffffffff
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}


def planes(s):
    p = [0, 0, 0]
    for i, ch in enumerate(s):
        c = CODE[ch]
        for k in range(3):
            p[k] |= ((c >> k) & 1) << i
    return p


def key(p, pos, j, g):
    gm = (1 << g) - 1
    return (j << 48) | (((p[2] >> pos) & gm) << 32) | (((p[1] >> pos) & gm) << 16) | ((p[0] >> pos) & gm)


def column_ed(B, m, A, n, d):
    """B (m letters) the pattern, A (n letters) the text, both as planes -> ed if it is <= d, else -1"""
    dl = m - n
    val = abs(dl)
    if val > d: return -1
    if m == 0 or n == 0: return val
    mm = (1 << m) - 1
    Pv, Mv = M64, 0
    for c in range(n):
        T = [M64 if (A[k] >> c) & 1 else 0 for k in range(3)]
        Eq = ~((B[0] ^ T[0]) | (B[1] ^ T[1]) | (B[2] ^ T[2])) & mm
        D0 = ((((Eq & Pv) + Pv) & M64) ^ Pv) | Eq | Mv
        Ph = (Mv | ~(D0 | Pv)) & M64
        Mh = Pv & D0
        row = c + 1 + dl
        if row >= 1: val += 1 - ((D0 >> (row - 1)) & 1)
        if val > d: return -1
        Ph = ((Ph << 1) | 1) & M64; Mh = (Mh << 1) & M64
        Pv = (Mh | ~(D0 | Ph)) & M64
        Mv = Ph & D0
    return val


def search(seqs, d, g):
    """-> (pairs [(i, j, dist)] ascending, verified [(i, j)] every pair that went through the column, in the order it did, candidates: the entries the tiles hold)"""
    N = len(seqs)
    P = [planes(s) for s in seqs]
    L = [len(s) for s in seqs]
    seedable = [L[s] >= (d + 1) * g for s in range(N)]
    entries = sorted(((key(P[s], j * g, j, g) if seedable[s] else NOKEY), s) for s in range(N) for j in range(d + 1))      # (key, sequence): sequences ascending within a key
    S = 2 * d + 1
    found, verified, candidates = [], [], 0
    gm = (1 << g) - 1
    for b in range(1, N):
        for q in range((d + 1) * S):
            j, s = q // S, q % S - d
            pos = j * g + s
            if pos < 0 or pos + g > L[b]: continue
            K = key(P[b], pos, j, g)
            lo = bisect.bisect_left(entries, (K, -1)); hi = bisect.bisect_left(entries, (K, b))
            for e in range(lo, hi):
                a = entries[e][1]
                candidates += 1
                first = True
                for q2 in range(q):
                    j2 = q2 // S; pos2 = j2 * g + q2 % S - d
                    if pos2 < 0 or pos2 + g > L[b]: continue
                    x = 0
                    for k in range(3): x |= (P[a][k] >> (j2 * g)) ^ (P[b][k] >> pos2)
                    if x & gm == 0: first = False
                if not first or abs(L[a] - L[b]) > d: continue
                verified.append((a, b))
                dist = column_ed(P[b], L[b], P[a], L[a], d)
                if dist >= 0: found.append((a, b, dist))
    # the short path: x not seedable against every y > x of a length within d
    order = sorted(range(N), key=lambda s: L[s])
    for x in range(N):
        if seedable[x]: continue
        for y in order:
            if y <= x or abs(L[y] - L[x]) > d: continue
            verified.append((x, y))
            dist = column_ed(P[x], L[x], P[y], L[y], d)
            if dist >= 0: found.append((x, y, dist))
    return sorted(found), verified, candidates
