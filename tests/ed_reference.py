"""A plain reference of the ngsid_ed_align_batch contract (include/ngsid.h, aln_mode 1), numpy only, written from the header and sharing
no code with oracle/ or the library - the anchor that oracle and kernel are both compared with (test anchors).

Contract: the whole query inside the target with unit costs, target ends free.  D is the full (n+1) x (m+1) int32 matrix with
D[0][j] = 0 and D[i][0] = i.  Two letters match only if both are A/C/G/T (either case) and equal; anything else matches nothing, itself
included.  End column = LEFTMOST minimum of the last row, distance = that value.  Traceback from (n, end): diagonal if
D[i-1][j-1] + neq == D[i][j], else up (a query-only column) if D[i-1][j] + 1 == D[i][j], else left.  span = {q_first, q_last, t_first,
t_last} over the diagonal columns (matches and mismatches), bp[w] the same over the diagonal columns whose target position t has
t // window == w, for w < bp_windows; -1 x 4 where there is none.  An empty query: distance 0, everything -1.
"""
import numpy as np

_CODE = np.full(256, 4, dtype=np.int8)
for _k, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _k; _CODE[ord(_c.lower())] = _k


def _codes(s):
    if isinstance(s, str): s = s.encode()
    return _CODE[np.frombuffer(bytes(s), dtype=np.uint8)]


def dp_matrix(q, t):
    """the full matrix, one vectorised row at a time: a[j] = min(diagonal, up) needs only the row above, and the left moves of a row are
    the min-scan cur[j] = min_k<=j (a[k] + j - k) = j + cummin(a[k] - k)"""
    qc, tc = _codes(q), _codes(t)
    n, m = len(qc), len(tc)
    D = np.zeros((n + 1, m + 1), dtype=np.int32)
    D[:, 0] = np.arange(n + 1, dtype=np.int32)
    col = np.arange(m + 1, dtype=np.int32)
    a = np.empty(m + 1, dtype=np.int32)
    for i in range(1, n + 1):
        prev = D[i - 1]
        neq = ((tc != qc[i - 1]) | (qc[i - 1] == 4)).astype(np.int32)       # (a target letter outside ACGT has code 4 and so never equals a query code < 4)
        a[0] = i
        np.minimum(prev[:-1] + neq, prev[1:] + 1, out=a[1:])
        D[i] = np.minimum.accumulate(a - col) + col
    return D


def traceback(D, q, t):
    """-> (distance, end column, diagonal columns as an int32 array [k, 2] of (query position, target position) in ascending order)"""
    qc, tc = _codes(q), _codes(t)
    n, m = len(qc), len(tc)
    end = int(np.argmin(D[n]))                                              # argmin returns the first = leftmost minimum
    dist = int(D[n, end])
    i, j = n, end
    cols = []
    while i > 0:
        if j > 0:
            neq = 0 if (qc[i - 1] < 4 and qc[i - 1] == tc[j - 1]) else 1
            if D[i - 1, j - 1] + neq == D[i, j]:
                cols.append((i - 1, j - 1)); i -= 1; j -= 1
                continue
        if D[i - 1, j] + 1 == D[i, j]:
            i -= 1
        else:
            j -= 1
    return dist, end, np.array(cols[::-1], dtype=np.int32).reshape(-1, 2)


def align_pair(q, t):
    D = dp_matrix(q, t)
    return traceback(D, q, t)


def outputs_of_path(dist, cols, window, bp_windows):
    """distance, span[4], bp[bp_windows, 4] from the diagonal columns of one alignment"""
    span = np.full(4, -1, dtype=np.int32)
    bp = np.full((bp_windows, 4), -1, dtype=np.int32)
    if len(cols):
        span[:] = (cols[0, 0], cols[-1, 0], cols[0, 1], cols[-1, 1])
        if bp_windows > 0:
            w = cols[:, 1] // window
            keep = w < bp_windows
            w = w[keep]; c = cols[keep]
            if len(w):
                first = np.ones(len(w), dtype=bool); first[1:] = w[1:] != w[:-1]        # target positions ascend, so each window is one run
                last = np.ones(len(w), dtype=bool); last[:-1] = first[1:]
                bp[w[first], 0] = c[first, 0]; bp[w[first], 2] = c[first, 1]
                bp[w[last], 1] = c[last, 0]; bp[w[last], 3] = c[last, 1]
    return dist, span, bp


def ed_align_batch(queries, targets, q_idx, t_idx, window=500, bp_windows=0, cache=None):
    """what api.ed_align_batch returns - distance[n], span[n, 4], bp[n, bp_windows, 4] (int32) - for lists of strings and index arrays.
    Every distinct (query, target) costs one DP; `cache` (a dict) keeps the paths across calls, whatever their windows."""
    if cache is None: cache = {}
    n = len(q_idx)
    dist = np.zeros(n, dtype=np.int32); span = np.zeros((n, 4), dtype=np.int32); bp = np.zeros((n, bp_windows, 4), dtype=np.int32)
    done = {}
    for p in range(n):
        key = (int(q_idx[p]), int(t_idx[p]))
        if key not in done:
            q, t = queries[key[0]], targets[key[1]]
            if (q, t) not in cache:
                d, _, cols = align_pair(q, t)
                cache[(q, t)] = (d, cols)
            done[key] = outputs_of_path(*cache[(q, t)], window, bp_windows)
        dist[p], span[p], bp[p] = done[key]
    return dist, span, bp


def last_row(q, t):
    """the last row of the matrix (for tests that ask how many columns attain its minimum)"""
    return dp_matrix(q, t)[-1]


# ---- the scalar form of the same contract: what the vectorised rows above are checked against (test_ed_reference_cpu.py)
def scalar_align_pair(q, t):
    ok = set("ACGTacgt")
    n, m = len(q), len(t)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        D[i][0] = i
        for j in range(1, m + 1):
            neq = 0 if (q[i - 1] in ok and t[j - 1] in ok and q[i - 1].upper() == t[j - 1].upper()) else 1
            D[i][j] = min(D[i - 1][j - 1] + neq, D[i - 1][j] + 1, D[i][j - 1] + 1)
    end = 0
    for j in range(1, m + 1):
        if D[n][j] < D[n][end]: end = j
    i, j, cols = n, end, []
    while i > 0:
        if j > 0:
            neq = 0 if (q[i - 1] in ok and t[j - 1] in ok and q[i - 1].upper() == t[j - 1].upper()) else 1
            if D[i - 1][j - 1] + neq == D[i][j]:
                cols.append((i - 1, j - 1)); i -= 1; j -= 1
                continue
        if D[i - 1][j] + 1 == D[i][j]: i -= 1
        else: j -= 1
    return D[n][end], end, cols[::-1]


def scalar_outputs(q, t, window, bp_windows):
    d, _, cols = scalar_align_pair(q, t)
    span = [-1] * 4; bp = [[-1] * 4 for _ in range(bp_windows)]
    for qi, ti in cols:
        if span[0] < 0: span[0] = qi; span[2] = ti
        span[1] = qi; span[3] = ti
        w = ti // window
        if w < bp_windows:
            if bp[w][0] < 0: bp[w][0] = qi; bp[w][2] = ti
            bp[w][1] = qi; bp[w][3] = ti
    return d, span, bp


# ---- one reference per test session: every test module that needs the answer of a case (ed_cases.Case) takes it from here
_paths = {}
_case_results = {}


def case_results(case):
    """(distance, span, bp) of one call of ed_cases; computed once, shared, and handed out read-only"""
    if case.name not in _case_results:
        r = ed_align_batch(case.queries, case.targets, case.q_idx, case.t_idx, case.window, case.bp_windows, cache=_paths)
        for a in r: a.setflags(write=False)
        _case_results[case.name] = r
    return _case_results[case.name]
