"""The blocked column of k_recruit (ngspeciesid_amd/csrc/k_recruit.hip) in Python integers - test infrastructure, not a test.

W = ceil(m / 64) words of 64 rows per pattern.  A column steps block 0, 1, ... in turn; block b hands its horizontal delta at its last row (hout: +1, -1 or 0) to
block b + 1 as hin, and the carry of the addition is NOT handed on.  The score is followed at row m - 1 of the last block.  tests/test_recruit_cpu.py checks the model
against the table of tests/recruit_reference.py on word-boundary cases.

The cut-off rule (edlib's last active block, made uniform over the lanes of a wave) is modelled beside it: only blocks 0 .. B are stepped.
  grow    before a column: if B is not the last block and SOME live lane has score(B) <= k, block B + 1 enters as all +1 vertical deltas (an upper bound of what it
          holds) with score(B + 1) = score(B) + rows(B + 1).  One block per column is enough: a cell of block B + 2 can be <= k in a column only if the last row of
          block B + 1 was <= k in the column before.
  shrink  after a column, one block at a time: if B > 0 and EVERY live lane has score(B) - (rows(B) - 1) > k - no cell of block B can be <= k -, block B leaves and
          score(B - 1) = score(B) - (sum of the vertical deltas of block B).
  score(b) is the value at the last row of block b; a lane is live while the column is inside its read.  s[j] is known where B is the last block; elsewhere it is
  above k.  Every cell whose true value is <= k lies in a stepped block and is exact there, so the hit, its distance and its end are those of the plain column."""
M64 = (1 << 64) - 1


def match_words(pattern: str):
    """{letter: [W words]}: bit i % 64 of word i // 64 is set where pattern[i] is the letter"""
    W = (len(pattern) + 63) // 64
    eq = {c: [0] * W for c in "ACGTN"}
    for i, c in enumerate(pattern):
        eq[c][i // 64] |= 1 << (i % 64)
    return eq


def step_block(Pv, Mv, Eq, hin, top):
    """one block, one text letter -> (Pv, Mv, hout); top = the bit of the block's last row"""
    hm = 1 if hin < 0 else 0
    hp = 1 if hin > 0 else 0
    Xv = Eq | Mv
    Eq2 = Eq | hm
    Xh = ((((Eq2 & Pv) + Pv) & M64) ^ Pv) | Eq2                         # the addition wraps at 64 bits: its carry stays in the block
    Ph = Mv | (~(Xh | Pv) & M64)
    Mh = Pv & Xh
    hout = ((Ph >> top) & 1) - ((Mh >> top) & 1)
    Ph = ((Ph << 1) | hp) & M64
    Mh = ((Mh << 1) | hm) & M64
    return Mh | (~(Xv | Ph) & M64), Ph & Xv, hout


def _rows(m, b):
    return min(64, m - 64 * b)


def last_row(pattern: str, read: str):
    """s[j] of the plain blocked column"""
    m = len(pattern); W = (m + 63) // 64
    eq = match_words(pattern)
    Pv, Mv = [M64] * W, [0] * W
    score, out = m, []
    for c in read:
        hin = 0
        for b in range(W):
            Pv[b], Mv[b], hin = step_block(Pv[b], Mv[b], eq[c][b], hin, _rows(m, b) - 1)
        score += hin
        out.append(score)
    return out


def locate(pattern: str, read: str, k: int):
    """(ed, end) or None from the plain column; k is already min(max_ed, m - 1)"""
    s = last_row(pattern, read)
    if not s or min(s) > k:
        return None
    return min(s), s.index(min(s))


def locate_cutoff(pattern: str, reads, k: int):
    """the lanes of one wave (reads) under the wave-uniform cut-off -> ([(ed, end) or None per read], block steps done, block steps of the plain column)"""
    m = len(pattern); W = (m + 63) // 64
    eq = match_words(pattern)
    n = len(reads)
    Pv = [[M64] * W for _ in range(n)]; Mv = [[0] * W for _ in range(n)]
    B = 0
    score = [_rows(m, 0)] * n                                           # at the last row of block B
    best = [None] * n
    done = 0
    Lmax = max([len(r) for r in reads], default=0)
    for j in range(Lmax):
        live = [x for x in range(n) if j < len(reads[x])]
        if B < W - 1 and any(score[x] <= k for x in live):              # grow
            B += 1
            for x in range(n):
                Pv[x][B], Mv[x][B] = M64, 0
                score[x] += _rows(m, B)
        for x in live:
            hin = 0
            for b in range(B + 1):
                Pv[x][b], Mv[x][b], hin = step_block(Pv[x][b], Mv[x][b], eq[reads[x][j]][b], hin, _rows(m, b) - 1)
            score[x] += hin
            if B == W - 1 and score[x] <= k and (best[x] is None or score[x] < best[x][0]):
                best[x] = (score[x], j)
        done += B + 1
        live = [x for x in live if j + 1 < len(reads[x])]               # the lanes that see another column
        if B > 0 and all(score[x] - (_rows(m, B) - 1) > k for x in live):         # shrink, one block per column
            for x in range(n):
                rows = (1 << _rows(m, B)) - 1
                score[x] -= bin(Pv[x][B] & rows).count("1") - bin(Mv[x][B] & rows).count("1")
            B -= 1
    return best, done, W * Lmax
