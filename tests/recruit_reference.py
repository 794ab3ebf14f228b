"""The definition of ngsid_recruit (include/ngsid_recruit.h) restated in numpy, independently of the kernel - test infrastructure, not a test.

The last row of the free-start edit-distance table is computed row by row: the diagonal and vertical moves are element-wise, the horizontal move
D[i][j] = min over j' <= j of (D'[i][j'] + j - j') is a running minimum of D'[i][j'] - j'.  Strands, bounds and the reduction follow the header word for word."""
import numpy as np

NONE = (-1, -1, 0, -1, -1, -1)                                   # cons, ed, strand, end, cons2, ed2 of a read with nothing

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s: str) -> str:
    return "".join(_COMP[c] for c in reversed(s))


def last_row(pattern: str, read: str) -> np.ndarray:
    """s[j] = D[m][j + 1], j = 0 .. L - 1; letters are equal iff their bytes are"""
    L = len(read)
    x = np.frombuffer(read.encode(), dtype=np.uint8)
    j = np.arange(L + 1, dtype=np.int64)
    prev = np.zeros(L + 1, dtype=np.int64)                               # D[0][j] = 0
    for i, c in enumerate(pattern.encode(), 1):
        cur = np.empty(L + 1, dtype=np.int64)
        cur[0] = i
        cur[1:] = np.minimum(prev[:-1] + (x != c), prev[1:] + 1)
        prev = np.minimum.accumulate(cur - j) + j                        # the horizontal move
    return prev[1:]


def locate(pattern: str, read: str, max_ed: int):
    """one pattern strand against one read -> (ed, end) or None: the minimum of the last row, its first position, a hit iff L > 0 and ed <= min(max_ed, m - 1)"""
    if not len(read):
        return None
    s = last_row(pattern, read)
    d = int(s.min())
    return (d, int(np.argmax(s == d))) if d <= min(int(max_ed), len(pattern) - 1) else None


def pair(cons: str, read: str, max_ed: int, both_strands=True):
    """one consensus against one read -> (D, strand, end) or None; a tie of the strands goes to forward"""
    best = None
    for strand, p in enumerate((cons, revcomp(cons)) if both_strands else (cons,)):
        h = locate(p, read, max_ed)
        if h is not None and (best is None or h[0] < best[0]):
            best = (h[0], strand, h[1])
    return best


def locate_many(pattern: str, reads, max_ed: int):
    """locate(pattern, r, max_ed) for every r of reads, the same rows computed for all reads at once: one table row is a [reads, columns] array, every read padded with a
    letter that equals nothing - a column depends only on the columns before it, so the padding behind a read's end changes nothing inside it"""
    n = len(reads)
    Lmax = max([len(r) for r in reads], default=0)
    assert len(pattern) + Lmax < 32000                                   # the rows are int16
    if n == 0 or Lmax == 0:
        return [None] * n
    x = np.zeros((n, Lmax), dtype=np.uint8)
    for i, r in enumerate(reads):
        x[i, :len(r)] = np.frombuffer(r.encode(), dtype=np.uint8)
    j = np.arange(Lmax + 1, dtype=np.int16)
    prev = np.zeros((n, Lmax + 1), dtype=np.int16)
    for i, c in enumerate(pattern.encode(), 1):
        cur = np.empty_like(prev)
        cur[:, 0] = i
        np.minimum(prev[:, :-1] + (x != c), prev[:, 1:] + 1, out=cur[:, 1:])
        prev = np.minimum.accumulate(cur - j, axis=1) + j
    k = min(int(max_ed), len(pattern) - 1)
    out = []
    for i, r in enumerate(reads):
        s = prev[i, 1:len(r) + 1]
        d = int(s.min()) if len(r) else k + 1
        out.append((d, int(np.argmax(s == d))) if d <= k else None)
    return out


def recruit(reads, read_off, cons, cons_off, max_ed, both_strands=True) -> np.ndarray:
    """-> hits [n, 6] int32"""
    hits = np.tile(np.array(NONE, dtype=np.int32), (len(reads), 1))
    for g in range(len(read_off) - 1):
        r0, r1 = int(read_off[g]), int(read_off[g + 1])
        per_cons = {}                                                    # c -> per read of the group (D, strand, end) or None; a tie of the strands goes to forward
        for c in range(int(cons_off[g]), int(cons_off[g + 1])):
            best = [None] * (r1 - r0)
            for strand, p in enumerate((cons[c], revcomp(cons[c])) if both_strands else (cons[c],)):
                for i, h in enumerate(locate_many(p, reads[r0:r1], max_ed[c])):
                    if h is not None and (best[i] is None or h[0] < best[i][0]):
                        best[i] = (h[0], strand, h[1])
            per_cons[c] = best
        for r in range(r0, r1):
            found = []                                                   # (D, index, strand, end)
            for c in range(int(cons_off[g]), int(cons_off[g + 1])):
                h = per_cons[c][r - r0]
                if h is not None:
                    found.append((h[0], c, h[1], h[2]))
            found.sort(key=lambda f: (f[0], f[1]))
            if found:
                hits[r, :4] = (found[0][1], found[0][0], found[0][2], found[0][3])
            if len(found) > 1:
                hits[r, 4:] = (found[1][1], found[1][0])
    return hits
