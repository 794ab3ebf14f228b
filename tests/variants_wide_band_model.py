"""Python-int model of the W-word band recurrence csrc/k_near.hip runs per lane for the wide calls (include/ngsid_near.h, near_band_ed_wide<W>), word for word: the
same letter planes in the same 32-bit layout, the same sliding register file of pattern words, the same carry from word to word, the same shift across words, the
same selection of the tracked bit and the same early exit.  Checked on the CPU against the full DP (test_variants_wide_band_model_cpu.py) before the kernel runs.
The one-word model is variants_band_model.py; the text planes (TEXT, TEXT_RC) are its planes, unchanged.

Frame.  A band of W 64-bit words, B = 64 W bits, H = B / 2 - 1 = 32 W - 1.  In column c (1-based) bit r of the band is row c - H + r, so a diagonal keeps its bit and
the cell (m, n) sits at bit H - (n - m); word j of the band holds bits 64 j .. 64 j + 63.  The band holds K = H edits exactly, by the argument of the one-word model.
The wide PATTERN planes are packed once for the widest band (PAD = 255 leading pad bits, base p at bit p + 255): the window of column c + 1 of a W-word band starts at
bit c + 255 - H = c + 32 (8 - W), a whole number of 32-bit words in.  A lane keeps 2 W + 1 words per plane for 32 columns and slides them by one word per block; the
word that enters is loaded one block ahead.
"""
import variants_band_model as bm

M32, M64 = bm.M32, bm.M64
WMAX = 8                                  # the widest instance: the pad of the wide pattern planes is 32 * WMAX - 1 bits
PAD_BITS = 32 * WMAX - 1
WIDTHS = (2, 4, 8)


def edits(W):
    """the edits a band of W words holds exactly"""
    return 32 * W - 1


def width_for(K):
    """the smallest instantiated W whose band holds K edits"""
    for W in WIDTHS:
        if K <= edits(W): return W
    raise ValueError("K = %d is beyond the widest band" % K)


def n_words_wide(length):
    """words per wide pattern plane: the bases, the eight pad words in front, the 2 W words a window spans beyond its first and the word loaded one block ahead,
    for texts up to 32 W - 1 bases longer than the pattern (read_bound() is the farthest word read)"""
    return ((length + 31) >> 5) + 3 * WMAX + 2


def read_bound(m, n, W):
    """the farthest wide pattern word the loop reads for a pattern of m and a text of n >= 1 bases: the word loaded ahead in the last block"""
    return (WMAX - W) + ((n - 1) >> 5) + 2 * W + 1


def pack_wide(seq):
    """-> three lists of n_words_wide(len) 32-bit words: plane k holds bit k of the code of base p at bit p + PAD_BITS, 7 (equals nothing) elsewhere"""
    nw = n_words_wide(len(seq))
    planes = [[0] * nw for _ in range(3)]
    for w in range(nw):
        for t in range(32):
            p = 32 * w + t - PAD_BITS
            c = bm.CODE[seq[p]] if 0 <= p < len(seq) else bm.PAD
            for k in range(3):
                planes[k][w] |= ((c >> k) & 1) << t
    return planes


def band_ed(pat, txt, m, n, K, W, info=None):
    """the lane's loop: pat = pack_wide(a), txt = bm.pack(b, TEXT or TEXT_RC) -> ed if it is <= K <= 32 W - 1, else -1.  info (a dict): 'columns' = columns computed,
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


def ed_within(a, b, K, W=None, both_strands=True):
    """(dist, strand) of include/ngsid_near.h through the model, the way the kernels call the loop: forward first, the reverse strand only below the forward result"""
    W = W or width_for(K)
    pat = pack_wide(a)
    f = band_ed(pat, bm.pack(b, bm.TEXT), len(a), len(b), K, W)
    if not both_strands or f == 0:
        return f, 0
    r = band_ed(pat, bm.pack(b, bm.TEXT_RC), len(a), len(b), K if f < 0 else f - 1, W)
    return (r, 1) if r >= 0 else (f, 0)
