"""The definition of ngsid_demux_scan (include/ngsid_demux.h) restated in numpy, and the cuts the policy of ngspeciesid_amd/demux.py has to make on hand-made cases -
test infrastructure, not a test.

The last row of the free-start edit-distance table is computed row by row: the diagonal and vertical moves are element-wise, the horizontal move
D[i][j] = min over j' <= j of (D'[i][j'] + j - j') is a running minimum of D'[i][j'] - j'.  Runs, hits and the CSR follow the header word for word."""
import functools
import numpy as np

_SETS = {"M": "AC", "R": "AG", "W": "AT", "S": "CG", "Y": "CT", "K": "GT", "V": "ACG", "H": "ACT", "D": "AGT", "B": "CGT", "X": "ACGT", "N": "ACGT"}


def letters_equal(a: str, b: str, iupac) -> bool:
    """the equality of ngsid_host_infix_locate: the same letter, or with iupac one letter's set holds the other letter (symmetric, not transitive)"""
    return a == b or (bool(iupac) and (b in _SETS.get(a, "") or a in _SETS.get(b, "")))


@functools.lru_cache(maxsize=None)
def _mismatch_table(c: str, iupac: bool) -> np.ndarray:
    return np.array([0 if letters_equal(c, chr(v), iupac) else 1 for v in range(256)], dtype=np.int64)


def last_row(pattern: str, read: str, iupac=True) -> np.ndarray:
    """s[j] = D[m][j + 1], j = 0 .. L - 1"""
    L = len(read)
    x = np.frombuffer(read.encode(), dtype=np.uint8)
    j = np.arange(L + 1, dtype=np.int64)
    prev = np.zeros(L + 1, dtype=np.int64)                               # D[0][j] = 0
    for i, c in enumerate(pattern, 1):
        neq = _mismatch_table(c, bool(iupac))[x]
        cur = np.empty(L + 1, dtype=np.int64)
        cur[0] = i
        cur[1:] = np.minimum(prev[:-1] + neq, prev[1:] + 1)
        cur = np.minimum.accumulate(cur - j) + j                         # the horizontal move
        prev = cur
    return prev[1:]


def runs_to_hits(s: np.ndarray, k: int):
    """[(end, ed)]: one per maximal interval of positions with s <= k; ed = the minimum over the interval, end = its first position with that value"""
    out = []
    ok = s <= k
    j, L = 0, len(s)
    while j < L:
        if not ok[j]:
            j += 1; continue
        a = j
        while j < L and ok[j]:
            j += 1
        ed = int(s[a:j].min())
        out.append((a + int(np.argmax(s[a:j] == ed)), ed))
    return out


def scan(reads, patterns, max_ed, iupac=True):
    """-> (hit_off [n + 1] uint64, hits [H, 3] int32 (pattern, end, ed)), within a read in ascending (end, pattern) order"""
    hit_off = np.zeros(len(reads) + 1, dtype=np.uint64)
    rows = []
    for r, read in enumerate(reads):
        mine = []
        for p, pat in enumerate(patterns):
            k = min(int(max_ed), len(pat) - 1)
            if len(read):
                mine += [(end, p, ed) for end, ed in runs_to_hits(last_row(pat, read, iupac), k)]
        mine.sort()
        rows += [(p, end, ed) for end, p, ed in mine]
        hit_off[r + 1] = len(rows)
    return hit_off, np.array(rows, dtype=np.int32).reshape(-1, 3)


def best_hit(hit_off, hits, r, p):
    """the hit of (read r, pattern p) with the smallest (ed, end) -> (ed, end) or None"""
    h = hits[int(hit_off[r]):int(hit_off[r + 1])]
    h = h[h[:, 0] == p]
    return min((int(d), int(e)) for _, e, d in h.tolist()) if len(h) else None


# ---- the policy's cuts on hand-made cases: (hits [k, 3], pattern lengths, number of tags T, read length L) -> the pieces the read is cut into
#      pattern p < T is tag p, pattern T + p its reverse complement
CUT_CASES = [
    # a forward tag of 10 letters ending at 59 with 0 edits: the amplicon to its right starts at 50
    dict(hits=[(0, 59, 0)], plen=[10, 10], T=1, L=100, cuts=[50], pieces=[(0, 50), (50, 100)]),
    # the same with 2 edits: the start is at 52 at the latest, the cut goes 2 further left
    dict(hits=[(0, 59, 2)], plen=[10, 10], T=1, L=100, cuts=[48], pieces=[(0, 48), (48, 100)]),
    # a reverse-complement pattern ends the amplicon to its left: cut behind it
    dict(hits=[(1, 59, 1)], plen=[10, 10], T=1, L=100, cuts=[60], pieces=[(0, 60), (60, 100)]),
    # a forward pattern whose estimated start lies before the read: clamped at 0, no piece to its left
    dict(hits=[(0, 8, 2)], plen=[10, 10], T=1, L=100, cuts=[0], pieces=[(0, 100)]),
    # two hits, one identical cut: the reverse complement ends at 49, the forward tag starts at 50
    dict(hits=[(1, 49, 0), (0, 59, 0)], plen=[10, 10], T=1, L=100, cuts=[50], pieces=[(0, 50), (50, 100)]),
    # junk between the two amplicons is a piece of its own
    dict(hits=[(1, 49, 0), (0, 69, 0)], plen=[10, 10], T=1, L=100, cuts=[50, 60], pieces=[(0, 50), (50, 60), (60, 100)]),
    # a reverse-complement pattern that ends at the last base cuts nothing off
    dict(hits=[(1, 99, 0)], plen=[10, 10], T=1, L=100, cuts=[100], pieces=[(0, 100)]),
]


def make_concatemers(pool, pairs):
    """reads pairs[i] = (a, b, ...) of a demux_reference.make_pool joined end to end -> (seqs, quals)"""
    return (["".join(pool["seqs"][i] for i in p) for p in pairs], ["".join(pool["quals"][i] for i in p) for p in pairs])
