"""Python-int model of the one-word band recurrence csrc/k_near.hip runs per lane (include/ngsid_near.h), word for word: the same letter planes in the same 32-bit
layout, the same sliding 64-bit windows, the same Hyyro step, the same tracked diagonal and the same early exit.  Checked on the CPU against the full DP
(test_variants_band_model_cpu.py) before the kernel ever runs.

Frame.  Pattern a (m rows), text b (n columns), D the full DP matrix.  In column c (1-based) bit r of a word is row c - 31 + r, so a diagonal of the matrix keeps its
bit from column to column and the cell (m, n) sits at bit 31 - (n - m).  Rows <= 0 are virtual rows that match nothing and hold D[i][c] = c; rows > m match nothing.
VP / VN are the vertical deltas of the column before, already aligned to the rows of the column that is computed (row c + 32 was outside the band before: its delta is
taken as +1, which can only raise a value).  Every band value is the cost of a real alignment, so it is >= D, and it equals D where D <= 31 (a path of cost <= 31
stays within 31 diagonals of the main one).  Values never decrease along a diagonal: a pair is dead as soon as the tracked value exceeds K.
"""
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
PAD = 7                                   # the code of a position outside the sequence: equals no letter
PATTERN, TEXT, TEXT_RC = 0, 1, 2          # the three variants k_near_pack writes per sequence


def n_words(length):
    """words per plane of a sequence of `length` bases: its bits, the pattern variant's 31 leading pad bits, and the two words a window reads ahead"""
    return ((length + 31) >> 5) + 3


def code_at(seq, variant, u):
    """the 3-bit code at bit u of a variant: PATTERN holds base p at bit p + 31, TEXT base p at bit p, TEXT_RC the complement of base len - 1 - p at bit p"""
    L = len(seq)
    p = u - 31 if variant == PATTERN else u
    if p < 0 or p >= L:
        return PAD
    if variant == TEXT_RC:
        c = CODE[seq[L - 1 - p]]
        return 3 - c if c < 4 else c
    return CODE[seq[p]]


def pack(seq, variant):
    """-> three lists of n_words(len) 32-bit words: plane k holds bit k of every code"""
    nw = n_words(len(seq))
    planes = [[0] * nw for _ in range(3)]
    for w in range(nw):
        for t in range(32):
            c = code_at(seq, variant, 32 * w + t)
            for k in range(3):
                planes[k][w] |= ((c >> k) & 1) << t
    return planes


def band_ed(pat, txt, m, n, K, info=None):
    """the lane's loop: pat = pack(a, PATTERN), txt = pack(b, TEXT or TEXT_RC) -> ed if it is <= K, else -1.  info (a dict): 'columns' = columns computed,
    'dead_at' = the column at which the pair was declared dead (None: never), 'diag' = the tracked values column by column"""
    d = n - m
    val = -d if d < 0 else 0
    if info is not None: info.update(columns=0, dead_at=None, diag=[])
    if abs(d) > K:
        if info is not None: info["dead_at"] = 0
        return -1
    sb = 31 - d
    VP, VN = (M64 << 31) & M64, 0
    for c0 in range(0, n, 32):
        w = c0 >> 5
        pw = [[pat[k][w], pat[k][w + 1], pat[k][w + 2]] for k in range(3)]
        tw = [txt[k][w] for k in range(3)]
        for s in range(min(32, n - c0)):
            ne = 0
            for k in range(3):
                lo = (((pw[k][1] << 32) | pw[k][0]) >> s) & M32
                hi = (((pw[k][2] << 32) | pw[k][1]) >> s) & M32
                win = (hi << 32) | lo
                mask = M64 if (tw[k] >> s) & 1 else 0
                ne |= win ^ mask
            Eq = ~ne & M64
            D0 = ((((Eq & VP) + VP) & M64) ^ VP) | Eq | VN
            HP = VN | (~(D0 | VP) & M64)
            HN = D0 & VP
            D0s = D0 >> 1
            VP = HN | (~(D0s | HP) & M64) | (1 << 63)
            VN = D0s & HP
            val += 1 - ((D0 >> sb) & 1)
            if info is not None: info["columns"] += 1; info["diag"].append(val)
            if val > K:
                if info is not None: info["dead_at"] = c0 + s + 1
                return -1
    return val


def ed_within(a, b, K, both_strands=True):
    """(dist, strand) of include/ngsid_near.h through the model, the way the kernels call the loop: forward first, the reverse strand only below the forward result"""
    pat = pack(a, PATTERN)
    f = band_ed(pat, pack(b, TEXT), len(a), len(b), K)
    if not both_strands or f == 0:
        return f, 0
    r = band_ed(pat, pack(b, TEXT_RC), len(a), len(b), K if f < 0 else f - 1)
    return (r, 1) if r >= 0 else (f, 0)
