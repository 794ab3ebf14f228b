"""A plain reference of the ngsid_sg_align_batch / ngsid_sg_align_cigar_batch contract (include/ngsid.h) under this build's traceback rules (DESIGN.md:
H prefers diag > E > F, E / F prefer extension, end cell = first maximum over the last row, then a strictly larger one over the last column), numpy
only, sharing no code with oracle/, the library, parasail_like.py or oracle/ref_shim/ - the anchor that the oracle and the three Gotoh kernels are
compared with (test anchors).

Contract: query = rows, target = columns, all four end gaps free, a gap of length l costs open + (l - 1) ext.  Three full (n+1) x (m+1) int32 matrices:
    H[i][j]  best score of an alignment of q[:i], t[:j];  H[0][j] = H[i][0] = 0
    E[i][j]  ... that ends in a column holding t[j-1] only ('D');  E[i][0] = minus infinity;  E[i][j] = max(E[i][j-1] - ext, H[i][j-1] - open)
    F[i][j]  ... that ends in a column holding q[i-1] only ('I');  F[0][j] = minus infinity;  F[i][j] = max(F[i-1][j] - ext, H[i-1][j] - open)
    H[i][j] = max(H[i-1][j-1] + s(q[i-1], t[j-1]), E[i][j], F[i][j])
s is case-insensitive over ACGT (match / mismatch); any other letter scores 0 against everything, itself included.  The matrices are filled by
anti-diagonals (cell (i, j) needs only i + j - 1 and i + j - 2), which is exact for any open and ext, open < ext and ext = 0 included; an anti-diagonal
of the row-major matrix is a strided slice, so every step is a handful of whole-array operations.

NO FLAGS are kept: the path is derived from the matrix VALUES.  From the end cell, in state H: the diagonal if H[i-1][j-1] + s == H[i][j], else E if
E[i][j] == H[i][j], else F.  In state E at (i, j): the column 'D', then the run continues in E at (i, j-1) while E[i][j-1] - ext >= H[i][j-1] - open, else
state H at (i, j-1); F alike along i.  What is left of the query or of the target when a border is reached, and what follows the end cell, are the free end
gaps ('I' / 'D'): at either end at most one of the two runs is non-empty, because the path starts on row 0 or column 0 and ends on row n or column m.
Columns: '=' raw bytes equal, 'X' raw bytes differ, 'I' query only, 'D' target only.  An empty query or target: n + m gap columns, score 0.
"""
from collections import namedtuple
import numpy as np

NEG = -(1 << 29)
_CODE = np.full(256, 4, dtype=np.int8)
for _k, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _k; _CODE[ord(_c.lower())] = _k

# kinds of tie a path can meet (Result.ties): the case conditions of align_cases family c are stated in these
DIAG_E, DIAG_F, E_F, EXT_OPEN_E, EXT_OPEN_F, ROW_COL, ROW_MULTI, COL_MULTI = "diag=E", "diag=F", "E=F", "ext=open in E", "ext=open in F", "row max=column max", "row max twice", "column max twice"

Result = namedtuple("Result", "score cols n_cols n_match span tie_cells ties end")


def _raw(s):
    if isinstance(s, str): s = s.encode()
    return np.frombuffer(bytes(s), dtype=np.uint8)


def matrices(q, t, match, mismatch, open_, ext):
    """-> H, E, F, each (n+1) x (m+1) int32; n, m >= 1"""
    qc, tc = _CODE[_raw(q)], _CODE[_raw(t)]
    n, m = len(qc), len(tc)
    W = m + 1
    H = np.zeros((n + 1, W), dtype=np.int32); E = np.full((n + 1, W), NEG, dtype=np.int32); F = np.full((n + 1, W), NEG, dtype=np.int32)
    h, e, f = H.reshape(-1), E.reshape(-1), F.reshape(-1)
    qs = np.where(qc < 4, qc, 5).astype(np.int8)             # a letter outside ACGT equals nothing: 5 on the query side, 4 on the target side
    wild_t = tc == 4
    for d in range(2, n + m + 1):
        lo, hi = max(1, d - m), min(n, d - 1)                # rows of anti-diagonal d; cell (i, d - i) sits at i * W + d - i = i * m + d
        a, b = lo * m + d, hi * m + d + 1
        tt = tc[d - hi - 1:d - lo][::-1]; qq = qs[lo - 1:hi]
        s = np.where(qq == tt, match, mismatch).astype(np.int32)
        s[(qq == 5) | wild_t[d - hi - 1:d - lo][::-1]] = 0
        ee = np.maximum(e[a - 1:b - 1:m] - ext, h[a - 1:b - 1:m] - open_)
        ff = np.maximum(f[a - W:b - W:m] - ext, h[a - W:b - W:m] - open_)
        e[a:b:m] = ee; f[a:b:m] = ff
        h[a:b:m] = np.maximum(np.maximum(h[a - W - 1:b - W - 1:m] + s, ee), ff)
    return H, E, F


def _sub(qc, tc, i, j, match, mismatch):
    a, b = qc[i - 1], tc[j - 1]
    return 0 if (a == 4 or b == 4) else (match if a == b else mismatch)


def align_pair(q, t, match=2, mismatch=-2, open_=3, ext=1):
    """-> Result of one pair: score, the column string (alignment order, end gaps included), n_cols, n_match, span, tie_cells, ties (set of kinds), end cell"""
    qr, tr = _raw(q), _raw(t)
    n, m = len(qr), len(tr)
    if n == 0 or m == 0:
        return Result(0, "I" * n + "D" * m, n + m, 0, (-1, -1, -1, -1), 0, frozenset(), (n, m))
    qc, tc = _CODE[qr], _CODE[tr]
    H, E, F = matrices(q, t, match, mismatch, open_, ext)
    row, col = H[n, 1:], H[1:, m]
    rbest, cbest = int(row.max()), int(col.max())
    ties = set(); tie_cells = 0
    if cbest > rbest: i, j, best = int(np.argmax(col)) + 1, m, cbest            # argmax: the first maximum
    else: i, j, best = n, int(np.argmax(row)) + 1, rbest
    # the end cell is a tie when the maximum is attained at more than one cell of the last row and the last column ((n, m) belongs to both)
    nrow = int((row == best).sum()); ncol = int((col[:-1] == best).sum())
    if nrow + ncol > 1:
        tie_cells += 1
        if nrow > 1: ties.add(ROW_MULTI)
        if ncol + (1 if row[-1] == best else 0) > 1: ties.add(COL_MULTI)
        if ncol >= 1 and int((row[:-1] == best).sum()) >= 1: ties.add(ROW_COL)
    end = (i, j)
    out = ["I"] * (n - i) + ["D"] * (m - j)                  # reverse order; one of the two runs is empty
    state = 0; q_first = q_last = t_first = t_last = -1; n_match = 0
    while i > 0 and j > 0:
        if state == 0:
            hv = int(H[i, j]); dg = int(H[i - 1, j - 1]) + _sub(qc, tc, i, j, match, mismatch) == hv; ev = int(E[i, j]) == hv; fv = int(F[i, j]) == hv
            if dg + ev + fv > 1:
                tie_cells += 1
                if dg and ev: ties.add(DIAG_E)
                if dg and fv: ties.add(DIAG_F)
                if ev and fv: ties.add(E_F)
            if dg:
                eq = qr[i - 1] == tr[j - 1]
                out.append("=" if eq else "X"); n_match += int(eq)
                if q_last < 0: q_last, t_last = i - 1, j - 1
                q_first, t_first = i - 1, j - 1
                i -= 1; j -= 1
            elif ev: state = 1
            else:
                assert fv, "no source reproduces H[%d][%d]" % (i, j)
                state = 2
        elif state == 1:
            out.append("D")
            x, o = int(E[i, j - 1]) - ext, int(H[i, j - 1]) - open_
            assert max(x, o) == int(E[i, j])
            if x == o: tie_cells += 1; ties.add(EXT_OPEN_E)
            if x < o: state = 0
            j -= 1
        else:
            out.append("I")
            x, o = int(F[i - 1, j]) - ext, int(H[i - 1, j]) - open_
            assert max(x, o) == int(F[i, j])
            if x == o: tie_cells += 1; ties.add(EXT_OPEN_F)
            if x < o: state = 0
            i -= 1
    out += ["I"] * i + ["D"] * j
    cols = "".join(reversed(out))
    return Result(best, cols, len(cols), n_match, (q_first, q_last, t_first, t_last), tie_cells, frozenset(ties), end)


def region(cols, k, match_id=None):
    """number of k-column windows with at least match_id '=' columns; ONE window (all columns) when n_cols < k - an empty alignment included"""
    if match_id is None: match_id = k
    c = np.concatenate(([0], np.cumsum(np.frombuffer(cols.encode(), dtype=np.uint8) == ord("="))))
    win = c[k:] - c[:-k] if len(cols) >= k else c[-1:]
    return int((win >= match_id).sum())


def sg_align_batch(queries, targets, q_idx, t_idx, open_, ext=1, match=2, mismatch=-2, k=13, match_id=None, cache=None):
    """what api.sg_align_batch returns (score, n_cols, n_match, region: int32 [n]) plus the column strings, the spans [n, 4] and the Result of every pair.
    `cache` (a dict) keeps the Result of (query, target, scheme) across calls."""
    if cache is None: cache = {}
    n = len(q_idx)
    open_ = np.broadcast_to(np.asarray(open_, dtype=np.int32), (n,)); mid = np.broadcast_to(np.asarray(k if match_id is None else match_id, dtype=np.int32), (n,))
    score = np.zeros(n, dtype=np.int32); ncols = np.zeros(n, dtype=np.int32); nmatch = np.zeros(n, dtype=np.int32); reg = np.zeros(n, dtype=np.int32); span = np.zeros((n, 4), dtype=np.int32)
    cols, res = [], []
    for p in range(n):
        q, t = queries[int(q_idx[p])], targets[int(t_idx[p])]
        key = (q, t, match, mismatch, int(open_[p]), ext)
        if key not in cache: cache[key] = align_pair(q, t, match, mismatch, int(open_[p]), ext)
        r = cache[key]
        score[p], ncols[p], nmatch[p], span[p] = r.score, r.n_cols, r.n_match, r.span
        reg[p] = region(r.cols, k, int(mid[p]))
        cols.append(r.cols); res.append(r)
    return score, ncols, nmatch, reg, cols, span, res


# ---- one reference per test session: every test module that needs the answer of a case (align_cases.Case) takes it from here
_pairs = {}
_case_results = {}


def case_results(case):
    """(score, n_cols, n_match, region, cols, span, results) of one call of align_cases; computed once, shared, and handed out read-only.  Pairs the case
    marks as oracle-only (case.ref[p] false) are not computed: their entries are 0 / '' / None."""
    if case.name not in _case_results:
        at = np.nonzero(case.ref)[0]
        r = sg_align_batch(case.queries, case.targets, case.q_idx[at], case.t_idx[at], case.open[at], case.ext, case.match, case.mismatch, case.k, case.match_id[at], cache=_pairs)
        n = len(case.q_idx); full = []
        for a in r[:4]: z = np.zeros(n, dtype=np.int32); z[at] = a; z.setflags(write=False); full.append(z)
        cols = [""] * n; res = [None] * n
        for x, p in enumerate(at): cols[p] = r[4][x]; res[p] = r[6][x]
        span = np.zeros((n, 4), dtype=np.int32); span[at] = r[5]; span.setflags(write=False)
        _case_results[case.name] = (full[0], full[1], full[2], full[3], tuple(cols), span, tuple(res))
    return _case_results[case.name]
