"""Python-int model of the W-word band recurrence csrc/k_near.hip runs per lane (include/ngsid_near.h, near_band_ed<W>), word for word, for W = 1, 2, 4 and 8: the
same letter planes in the same 32-bit layout, the same sliding register file of pattern words, the same carry from word to word, the same shift across words, the
same selection of the tracked bit and the same early exit; for W = 1 the kernel's one-word body (_one_word), which loads a block's words at its start.  Checked
on the CPU against the full DP (test_variants_band_model_cpu.py) before the kernel ever runs.

Frame.  Pattern a (m rows), text b (n columns), D the full DP matrix.  A band of W 64-bit words, B = 64 W bits, H = B / 2 - 1 = 32 W - 1.  In column c (1-based) bit r
of the band is row c - H + r, so a diagonal of the matrix keeps its bit from column to column and the cell (m, n) sits at bit H - (n - m); word j of the band holds
bits 64 j .. 64 j + 63.  Rows <= 0 are virtual rows that match nothing and hold D[i][c] = c; rows > m match nothing.  VP / VN are the vertical deltas of the column
before, already aligned to the rows of the column that is computed (row c + H + 1 was outside the band before: its delta is taken as +1, which can only raise a
value).  Every band value is the cost of a real alignment, so it is >= D, and it equals D where D <= H (a path of cost <= H stays within H diagonals of the main
one): the band holds K = H edits exactly.  Values never decrease along a diagonal: a pair is dead as soon as the tracked value exceeds K.
The pattern planes are packed once for the widest band (PAD_BITS = 255 leading pad bits, base p at bit p + 255): the window of column c + 1 of a W-word band starts at
bit c + 255 - H = c + 32 (8 - W), a whole number of 32-bit words in.  A lane keeps 2 W + 1 words per plane for 32 columns and slides them by one word per block; the
word that enters, and the next text word, are loaded one block ahead.  (In memory the kernel interleaves the three planes of a kind word by word; the model keeps
them as three lists of the same words.)
"""
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
PAD = 7                                   # the code of a position outside the sequence: equals no letter
TEXT, TEXT_RC = 0, 1                      # the two variants of the text planes k_near_pack writes per sequence
WMAX = 8                                  # the widest instance: the pad of the pattern planes is 32 * WMAX - 1 bits
PAD_BITS = 32 * WMAX - 1
WIDTHS = (1, 2, 4, 8)


def edits(W):
    """the edits a band of W words holds exactly"""
    return 32 * W - 1


def width_for(K):
    """the smallest instantiated W whose band holds K edits"""
    for W in WIDTHS:
        if K <= edits(W): return W
    raise ValueError("K = %d is beyond the widest band" % K)


def n_words(length):
    """words per text plane of a sequence of `length` bases: its bits and the word loaded one block ahead"""
    return ((length + 31) >> 5) + 1


def n_words_wide(length):
    """words per pattern plane: the bases, the eight pad words in front, the 2 W words a window spans beyond its first and the word loaded one block ahead,
    for texts up to 32 W - 1 bases longer than the pattern (read_bound() is the farthest word read)"""
    return ((length + 31) >> 5) + 3 * WMAX + 2


def read_bound(m, n, W):
    """the farthest pattern word the loop reads for a pattern of m and a text of n >= 1 bases: the word loaded ahead in the last block (W = 1 loads nothing ahead:
    the third word of the last block)"""
    return (WMAX - W) + ((n - 1) >> 5) + 2 * W + (1 if W > 1 else 0)


def _planes(nw, code_at):
    planes = [[0] * nw for _ in range(3)]
    for w in range(nw):
        for t in range(32):
            c = code_at(32 * w + t)
            for k in range(3):
                planes[k][w] |= ((c >> k) & 1) << t
    return planes


def pack(seq, variant):
    """the text planes -> three lists of n_words(len) 32-bit words: plane k holds bit k of every code; TEXT holds base p at bit p, TEXT_RC the complement of base
    len - 1 - p at bit p, 7 (equals nothing) elsewhere"""
    L = len(seq)
    def code_at(p):
        if p >= L: return PAD
        if variant == TEXT: return CODE[seq[p]]
        c = CODE[seq[L - 1 - p]]
        return 3 - c if c < 4 else c
    return _planes(n_words(L), code_at)


def pack_wide(seq):
    """the pattern planes -> three lists of n_words_wide(len) 32-bit words: plane k holds bit k of the code of base p at bit p + PAD_BITS, 7 elsewhere"""
    return _planes(n_words_wide(len(seq)), lambda u: CODE[seq[u - PAD_BITS]] if 0 <= u - PAD_BITS < len(seq) else PAD)


def band_ed(pat, txt, m, n, K, W, info=None):
    """the lane's loop: pat = pack_wide(a), txt = pack(b, TEXT or TEXT_RC) -> ed if it is <= K <= 32 W - 1, else -1.  info (a dict): 'columns' = columns computed,
    'dead_at' = the column at which the pair was declared dead (None: never), 'diag' = the tracked values, 'far' = the farthest pattern word read,
    'carries' = the number of columns in which a carry crossed from one word to the next"""
    H = 32 * W - 1
    assert 0 <= K <= H
    d = n - m
    val = -d if d < 0 else 0
    if info is not None: info.update(columns=0, dead_at=None, diag=[], far=-1, carries=0)
    if abs(d) > K:
        if info is not None: info["dead_at"] = 0
        return -1
    sb = H - d
    sw, sbit = sb >> 6, sb & 63
    VP = [0 if j < (H >> 6) else ((M64 << (H & 63)) & M64 if j == (H >> 6) else M64) for j in range(W)]
    VN = [0] * W
    if n == 0: return val
    if W == 1: return _one_word(pat, txt, n, K, sb, val, info)
    off = WMAX - W
    a = [[pat[k][off + i] for i in range(2 * W + 1)] for k in range(3)]
    t = [txt[k][0] for k in range(3)]
    for c0 in range(0, n, 32):
        w = c0 >> 5
        nxt = [pat[k][off + w + 2 * W + 1] for k in range(3)]            # loaded one block ahead
        tn = [txt[k][w + 1] for k in range(3)]
        if info is not None: info["far"] = max(info["far"], off + w + 2 * W + 1)
        for s in range(min(32, n - c0)):
            T = [M32 if (t[k] >> s) & 1 else 0 for k in range(3)]
            Eq = []
            for j in range(W):
                ne = [0, 0]
                for k in range(3):
                    lo = (((a[k][2 * j + 1] << 32) | a[k][2 * j]) >> s) & M32
                    hi = (((a[k][2 * j + 2] << 32) | a[k][2 * j + 1]) >> s) & M32
                    ne[0] |= lo ^ T[k]; ne[1] |= hi ^ T[k]
                Eq.append(~((ne[1] << 32) | ne[0]) & M64)
            D0, cy, crossed = [], 0, False
            for j in range(W):
                total = (Eq[j] & VP[j]) + VP[j] + cy
                cy = total >> 64
                if cy and j + 1 < W: crossed = True
                D0.append(((total & M64) ^ VP[j]) | Eq[j] | VN[j])
            for j in range(W):
                HP = VN[j] | (~(D0[j] | VP[j]) & M64)
                HN = D0[j] & VP[j]
                D0s = (D0[j] >> 1) | (((D0[j + 1] << 63) & M64) if j + 1 < W else 0)
                VP[j] = HN | (~(D0s | HP) & M64) | ((1 << 63) if j == W - 1 else 0)
                VN[j] = D0s & HP
            tr = D0[0]
            for j in range(1, W):
                if sw == j: tr = D0[j]
            val += 1 - ((tr >> sbit) & 1)
            if info is not None:
                info["columns"] += 1; info["diag"].append(val); info["carries"] += crossed
            if val > K:
                if info is not None: info["dead_at"] = c0 + s + 1
                return -1
        for k in range(3):
            a[k] = a[k][1:] + [nxt[k]]
            t[k] = tn[k]
    return val


def _one_word(pat, txt, n, K, sb, val, info):
    """the W = 1 body of the lane's loop: one 64-bit word, the three pattern words and the text word of a block loaded at its start, the windows as 64-bit shifts of
    word pairs; no carry, no shift across words, no selection of the tracked word"""
    off = WMAX - 1
    VP, VN = (M64 << 31) & M64, 0
    for c0 in range(0, n, 32):
        w = c0 >> 5
        pw = [[pat[k][off + w], pat[k][off + w + 1], pat[k][off + w + 2]] for k in range(3)]
        tw = [txt[k][w] for k in range(3)]
        if info is not None: info["far"] = max(info["far"], off + w + 2)
        for s in range(min(32, n - c0)):
            ne = 0
            for k in range(3):
                lo = (((pw[k][1] << 32) | pw[k][0]) >> s) & M32
                hi = (((pw[k][2] << 32) | pw[k][1]) >> s) & M32
                ne |= ((hi << 32) | lo) ^ (M64 if (tw[k] >> s) & 1 else 0)
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


def ed_within(a, b, K, W=None, both_strands=True):
    """(dist, strand) of include/ngsid_near.h through the model, the way the kernels call the loop: forward first, the reverse strand only below the forward result"""
    W = W or width_for(K)
    pat = pack_wide(a)
    f = band_ed(pat, pack(b, TEXT), len(a), len(b), K, W)
    if not both_strands or f == 0:
        return f, 0
    r = band_ed(pat, pack(b, TEXT_RC), len(a), len(b), K if f < 0 else f - 1, W)
    return (r, 1) if r >= 0 else (f, 0)
