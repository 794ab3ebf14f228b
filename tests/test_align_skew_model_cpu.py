"""The skewed gap frame of the paired int16 aligner (csrc/k_align16p.hip, SKEW instances), as a model on the CPU.

The kernel keeps every value of DP cell (i, j) as X^ = X + (i + j) ext with the row state g' = H - open + ext, which removes the two "- ext" of a cell:
    E^ = max(E^left, g'^left)    F^ = max(F^up, g'^up)    d^ = g'^diag + (score + open + ext)    h^ = max(d^, E^, F^)    g'^ = h^ - (open - ext)
and takes its four traceback flags as SIGN bits of int16 differences (d^ - h^, E^ - mx^, E^left - E^, F^up - F^).  The model below runs the plain recurrence of the
kernel (row state g = H - open, flags by comparison, 64-bit) and the skewed one in WRAPPING int16 with sign-bit flags, both with the kernel's border values (H = 0 in
row / column -1, E and F at NEG16 there, never lowered), one anti-diagonal at a time, and demands the same flags and the same H in every cell.
The second test is the range argument of the host's choice of the instance (ngsid_align16p_skew_exact, sg16p_flag_span in k_align_common.h): at the edge of that
bound the largest value, the smallest value and the largest same-cell difference of the skewed frame stay inside int16.
"""
import numpy as np

NEG16 = -20000
LET = np.frombuffer(b"ACGT", dtype=np.uint8)


def flag_span(match, ext, open_, qlen, tlen, skew):
    """sg16p_flag_span of k_align_common.h"""
    return -NEG16 + ext + open_ + match * min(qlen, tlen) + ((qlen + tlen + 1) * ext if skew else 0)


def _scores(q, t, match, mismatch):
    code = np.full(256, 4, dtype=np.int64); code[LET] = np.arange(4)
    a = code[q][:, None]; b = code[t][None, :]
    return np.where((a > 3) | (b > 3), 0, np.where(a == b, match, mismatch)).astype(np.int64)


def model(q, t, match, mismatch, open_, ext, skew, dtype=np.int64):
    """-> flags [n, m] (bit f = complement flag f of the kernel: 0 h != d, 1 mx != E, 2 E opened, 3 F opened), H [n, m] (plain frame), and, for the 64-bit runs, the
    extremes (largest value, smallest value above NEG16, largest same-cell difference in magnitude)"""
    n, m = len(q), len(t)
    S = _scores(q, t, match, mismatch)
    sk = ext if skew else 0
    wrap = dtype is np.int16
    # matrices with a border: index (i + 1, j + 1)
    G = np.zeros((n + 1, m + 1), dtype=dtype); E = np.full((n + 1, m + 1), NEG16, dtype=dtype); F = np.full((n + 1, m + 1), NEG16, dtype=dtype)
    ii = np.arange(-1, n, dtype=np.int64); jj = np.arange(-1, m, dtype=np.int64)
    G[:, 0] = (-open_ + sk + (ii - 1) * sk).astype(dtype)              # H = 0 in column -1: g' = -open + ext in the frame of cell (i, -1)
    G[0, :] = (-open_ + sk + (jj - 1) * sk).astype(dtype)              # and in row -1
    dk = dtype(open_ + sk); gsub = dtype(open_ - sk); ex = dtype(0 if skew else ext)
    flags = np.zeros((n, m), dtype=np.uint8); H = np.zeros((n, m), dtype=np.int64)
    vmax, vmin, dmax = -(1 << 40), 1 << 40, 0
    with np.errstate(over="ignore"):
        for k in range(n + m - 1):
            I = np.arange(max(0, k - m + 1), min(n - 1, k) + 1); Jc = k - I
            e_left = E[I + 1, Jc]; g_left = G[I + 1, Jc]; f_up = F[I, Jc + 1]; g_up = G[I, Jc + 1]; g_diag = G[I, Jc]
            e_ext = (e_left - ex).astype(dtype); f_ext = (f_up - ex).astype(dtype)
            Ev = np.maximum(e_ext, g_left); Fv = np.maximum(f_ext, g_up)
            d = (g_diag + (S[I, Jc].astype(dtype) + dk)).astype(dtype)
            mx = np.maximum(Ev, Fv); h = np.maximum(d, mx); g = (h - gsub).astype(dtype)
            diffs = [(d - h).astype(dtype), (Ev - mx).astype(dtype), (e_ext - Ev).astype(dtype), (f_ext - Fv).astype(dtype)]
            if wrap: fl = [(x < 0) for x in diffs]                      # the kernel: sign bits of packed 16-bit differences
            else: fl = [d != h, Ev != mx, e_ext != Ev, f_ext != Fv]    # the definition
            flags[I, Jc] = fl[0] | (fl[1] << 1) | (fl[2] << 2) | (fl[3] << 3)
            H[I, Jc] = g.astype(np.int64) + open_ - sk - k * sk
            E[I + 1, Jc + 1] = Ev; F[I + 1, Jc + 1] = Fv; G[I + 1, Jc + 1] = g
            if not wrap:
                vals = np.concatenate([e_left, g_left, f_up, g_up, g_diag, Ev, Fv, d, h, g])
                vmax = max(vmax, int(vals.max())); vmin = min(vmin, int(vals[vals > NEG16].min()))
                dmax = max(dmax, max(int(np.abs(x).max()) for x in diffs))
    return flags, H, (vmax, vmin, dmax)


def _mutate(rng, s, rate):
    out = []
    for c in s:
        u = rng.random()
        if u < rate * 0.4: out.append(int(LET[rng.integers(0, 4)]))
        elif u < rate * 0.7: continue
        elif u < rate: out.append(int(c)); out.append(int(LET[rng.integers(0, 4)]))
        else: out.append(int(c))
    return np.array(out if out else [int(LET[0])], dtype=np.uint8)


def _pair(rng, kind):
    n = int(rng.integers(1, 48))
    if kind == 0: base = LET[rng.integers(0, 4, n)]                                                   # random
    elif kind == 1:                                                                                  # homopolymer runs
        base = np.concatenate([np.full(int(rng.integers(1, 9)), LET[rng.integers(0, 4)], dtype=np.uint8) for _ in range(n)])[:n]
    else: unit = LET[rng.integers(0, 4, int(rng.integers(1, 5)))]; base = np.tile(unit, n)[:n]        # tandem repeat
    q = _mutate(rng, base, float(rng.choice([0.0, 0.1, 0.3])))
    t = _mutate(rng, base, float(rng.choice([0.0, 0.1, 0.3]))) if rng.random() < 0.8 else LET[rng.integers(0, 4, int(rng.integers(1, 48)))]
    if rng.random() < 0.2: t = np.concatenate([LET[rng.integers(0, 4, int(rng.integers(1, 20)))], t])    # overhangs
    if rng.random() < 0.2: q = np.concatenate([q, LET[rng.integers(0, 4, int(rng.integers(1, 20)))]])
    if rng.random() < 0.1: q = q.copy(); q[rng.integers(0, len(q))] = ord("N")                             # wildcards score 0
    return q, t


def test_skewed_frame_gives_the_flags_and_scores_of_the_plain_one():
    """match 0 - 4, mismatch 0 .. -8, ext 0 - 4, open 0 - 16 (open < ext and ext = 0 included) on random, homopolymer and tandem-repeat pairs: their ties are diagonal
    against gap, E against F and open against extend"""
    rng = np.random.default_rng(20)
    params = [(2, -2, 3, 1), (2, -2, 2, 0), (4, -8, 1, 4), (0, 0, 0, 0), (1, -1, 0, 2), (4, -8, 16, 4), (3, 0, 5, 0), (0, -3, 2, 3)]
    cells = 0
    for it in range(300):
        q, t = _pair(rng, it % 3)
        if it < len(params): match, mismatch, open_, ext = params[it]
        else: match, mismatch, open_, ext = int(rng.integers(0, 5)), -int(rng.integers(0, 9)), int(rng.integers(0, 17)), int(rng.integers(0, 5))
        fa, ha, _ = model(q, t, match, mismatch, open_, ext, skew=False)
        fb, hb, _ = model(q, t, match, mismatch, open_, ext, skew=True, dtype=np.int16)
        ctx = "pair %d (n %d, m %d) match %d mismatch %d open %d ext %d" % (it, len(q), len(t), match, mismatch, open_, ext)
        assert np.array_equal(fa, fb), "flags differ: " + ctx
        assert np.array_equal(ha, hb), "H differs: " + ctx
        cells += fa.size
    assert cells > 100000


def _edge_pairs(rng, n, m):
    q = LET[rng.integers(0, 4, n)]
    perfect = np.concatenate([LET[rng.integers(0, 4, m - n)], q])                      # the whole query at the END of the target: the largest score in the last cell
    unrelated = LET[rng.integers(0, 4, m)]
    overhang = np.concatenate([q[: n // 2], LET[rng.integers(0, 4, m - n // 2)]])      # half the query matches, the rest of the target hangs over
    return [(q, perfect), (q, unrelated), (q, overhang)]


def test_skewed_frame_stays_inside_int16_at_the_edge_of_the_predicate():
    """the corner of the 16-bit aligners (match 4, mismatch -8, open 16, ext 4) with the longest paired query and the longest target the bound admits, and ext = 1
    with the longest target of the 16-bit path: the extremes of the frame against the bound, and the wrapping int16 run against the plain one"""
    rng = np.random.default_rng(21)
    n = 896
    m4 = max(m for m in range(n, 4001) if flag_span(4, 4, 16, n, m, True) < 32768)
    assert flag_span(4, 4, 16, n, m4 + 1, True) >= 32768 and m4 > n                   # just inside
    assert flag_span(4, 1, 16, n, 4000, True) < 32768                                 # ext = 1: every length of the paired classes
    cases = [(4, -8, 16, 4, p) for p in _edge_pairs(rng, n, m4)] + [(4, -8, 16, 1, _edge_pairs(rng, n, 4000)[2])]
    for match, mismatch, open_, ext, (q, t) in cases:
        fa, ha, _ = model(q, t, match, mismatch, open_, ext, skew=False)
        fs, hs, (vmax, vmin, dmax) = model(q, t, match, mismatch, open_, ext, skew=True)
        fb, hb, _ = model(q, t, match, mismatch, open_, ext, skew=True, dtype=np.int16)
        bound = flag_span(match, ext, open_, len(q), len(t), True)
        assert bound < 32768
        assert vmax <= match * min(len(q), len(t)) + (len(q) + len(t)) * ext and vmax <= 32767
        assert vmin >= -2 * open_ - ext + mismatch and vmin > NEG16
        assert dmax <= bound - 1 and vmax - NEG16 <= bound - 1
        assert np.array_equal(fa, fs) and np.array_equal(ha, hs)
        assert np.array_equal(fa, fb) and np.array_equal(ha, hb)
    assert int(ha.max()) >= 0
