"""The skewed gap frame of the paired int16 aligner (csrc/k_align16p.hip, SKEW instances; ngsid_ctx_option align_skew, default 1): every value of cell (i, j) is
kept as X + (i + j) ext, which saves the two gap-extension subtractions of a cell, and the score of a row comes from a per-step byte table.  Same traceback words, so
the same outputs by pair index as the plain instances (align_skew = 0), the one-pair kernel (align_paired = 0) and the oracle.  The frame is undone in the maxima over
the last row and the last column, so the cases aim at the end cell (overhangs on both sides), at every row of a lane that can own the last query row (every residue
(n - 1) mod R of the four classes), at scoring parameters on both sides of the table's condition, and at the lengths where the host switches between the instances.
The arithmetic of the frame itself is modelled in test_align_skew_model_cpu.py.
"""
import ctypes as C
import numpy as np
import pytest
from ngspeciesid_amd._capi import ReadSet

pytestmark = pytest.mark.gpu
LET = np.frombuffer(b"ACGT", dtype=np.uint8)
NAMES = ("score", "ncols", "nmatch", "region")
CLASSES = ((4, 200, 256), (8, 400, 512), (12, 700, 768), (14, 790, 896))     # rows per lane, lowest and highest query length used in the class
NEG16 = -20000


def _opt(api, name, v):
    assert api.lib.ngsid_ctx_option(api.ctx, name, C.c_int64(v)) == 0


def _span(match, ext, open_, qlen, tlen):
    """sg16p_flag_span(..., skew) of k_align_common.h: the host runs the skewed instances while this is below 2^15"""
    return -NEG16 + ext + open_ + match * min(qlen, tlen) + (qlen + tlen + 1) * ext


def _mutate(rng, s, rate):
    u = rng.random(len(s)); out = []
    for c, x in zip(s.tolist(), u.tolist()):
        if x < rate * 0.4: out.append(int(LET[rng.integers(0, 4)]))
        elif x < rate * 0.7: continue
        elif x < rate: out.append(c); out.append(int(LET[rng.integers(0, 4)]))
        else: out.append(c)
    return np.array(out, dtype=np.uint8)


def _homopolymers(rng, n):
    runs = rng.integers(1, 12, n); return np.repeat(LET[rng.integers(0, 4, n)], runs)[:n]


def _tandem(rng, n):
    unit = LET[rng.integers(0, 4, int(rng.integers(1, 7)))]
    return np.tile(unit, n // len(unit) + 1)[:n]


def _fit(rng, q, n):
    """q cut or padded (with its own letters) to exactly n bases"""
    if len(q) >= n: return q[:n]
    return np.concatenate([q, q[rng.integers(0, len(q), n - len(q))]])


def _readset(seqs):
    return ReadSet(np.concatenate(seqs), None, np.concatenate(([0], np.cumsum([len(x) for x in seqs]))).astype(np.uint64))


def _make_batch(seed):
    """about 4 200 pairs of 200 - 896 bases: every residue (n - 1) mod R of every class, an odd number of pairs on the odd residues (a bin whose last item holds one
    pair), homopolymer and tandem-repeat pairs, overhangs of the target and of the query on both sides, a few pairs with N in the query or in the target"""
    rng = np.random.default_rng(seed)
    qs, ts = [], []
    for R, lo, hi in CLASSES:
        for res in range(R):
            n_first = lo + ((res - (lo - 1)) % R)
            lens = np.arange(n_first, hi + 1, R)
            for rep in range(int(rng.integers(40, 60)) * 2 + (res & 1)):
                n = int(lens[rep % len(lens)]) if rep < len(lens) else int(rng.choice(lens))
                kind = rng.random()
                if kind < 0.3: base = _homopolymers(rng, n + 40)
                elif kind < 0.6: base = _tandem(rng, n + 40)
                else: base = LET[rng.integers(0, 4, n + 40)]
                t = _mutate(rng, base, float(rng.choice([0.0, 0.03, 0.12])))
                q = _fit(rng, _mutate(rng, base, float(rng.choice([0.0, 0.05, 0.15]))), n)
                u = rng.random()
                if u < 0.1: t = t[int(rng.integers(1, 80)):]                                                  # the query hangs over on the left
                elif u < 0.2: t = np.concatenate([LET[rng.integers(0, 4, int(rng.integers(1, 120)))], t])     # the target hangs over on the left
                elif u < 0.3: t = np.concatenate([t, LET[rng.integers(0, 4, int(rng.integers(1, 120)))]])     # ... on the right (the end cell lies in the last row)
                elif u < 0.4: t = t[: len(t) - int(rng.integers(41, 120))]                                    # the query hangs over on the right (... in the last column)
                u = rng.random()
                if u < 0.04: q = q.copy(); q[rng.integers(0, n, 2)] = ord("N")
                elif u < 0.08: t = t.copy(); t[rng.integers(0, len(t), 2)] = ord("N")
                qs.append(q); ts.append(t)
    while len(qs) < 4200:
        n = 713; base = _tandem(rng, n + 20); qs.append(_fit(rng, _mutate(rng, base, 0.05), n)); ts.append(_mutate(rng, base, 0.05))
    return _readset(qs), _readset(ts), np.arange(len(qs), dtype=np.uint32), np.array([len(q) for q in qs])


@pytest.fixture(scope="module")
def batch():
    return _make_batch(51)


def _three(api, Q, T, qi, ti, opens, **kw):
    """align_skew 1, align_skew 0, align_paired 0"""
    try:
        _opt(api, b"align_paired", 1); _opt(api, b"align_skew", 1); a = api.sg_align_batch(Q, T, qi, ti, opens, **kw)
        _opt(api, b"align_skew", 0); b = api.sg_align_batch(Q, T, qi, ti, opens, **kw)
        _opt(api, b"align_paired", 0); c = api.sg_align_batch(Q, T, qi, ti, opens, **kw)
    finally:
        _opt(api, b"align_paired", 1); _opt(api, b"align_skew", 1)
    return a, b, c


def _same(a, b, what, qlen=None):
    for x, y, nm in zip(a, b, NAMES):
        bad = np.nonzero(x != y)[0]
        assert len(bad) == 0, "%s: %s differs at pairs %s%s" % (what, nm, bad[:8].tolist(), "" if qlen is None else " (query lengths %s)" % qlen[bad[:8]].tolist())


# match, mismatch, ext, lowest and highest open
PARAMS = {
    "clustering": (2, -2, 1, 2, 5),            # the table form: mismatch + open + ext >= 0
    "large_frame": (4, -8, 4, 4, 16),          # the corner of the 16-bit aligners; open 4 .. 7 have mismatch + open + ext < 0: items of both forms
    "ext0": (2, -2, 0, 2, 5),                  # no frame at all
    "open_below_ext": (2, -2, 3, 0, 2),        # a gap's first base is cheaper than its later ones
    "negative_mismatch_constant": (2, -8, 1, 1, 1),      # mismatch + open + ext < 0 in every pair: the skewed frame with the multiply-add score
}


@pytest.mark.parametrize("name", list(PARAMS))
def test_skewed_instances_equal_plain_ones_one_pair_kernel_and_oracle(gpu_api, oracle, batch, name):
    Q, T, idx, qlen = batch
    match, mismatch, ext, olo, ohi = PARAMS[name]
    tmax = int(np.diff(T.off.astype(np.int64)).max())
    assert _span(match, ext, ohi, 896, tmax) < 32768                   # this call is one the host gives to the skewed instances
    opens = np.random.default_rng(len(name)).integers(olo, ohi + 1, len(idx)).astype(np.int32)      # differs inside an item
    kw = dict(ext=ext, match=match, mismatch=mismatch, k=13)
    a, b, c = _three(gpu_api, Q, T, idx, idx, opens, **kw)
    _same(a, b, "align_skew 1 / 0", qlen)
    _same(a, c, "align_skew 1 / align_paired 0", qlen)
    pick = []                                                          # the oracle on the first, a middle and the last residue of each class, and on pairs with N
    for R, lo, hi in CLASSES:
        cls = np.nonzero((qlen >= lo) & (qlen <= hi))[0]
        for res in (0, R // 2, R - 1):
            pick.extend(cls[(qlen[cls] - 1) % R == res][:8].tolist())
    pick = np.array(sorted(set(pick)), dtype=np.int64)
    o = oracle.sg_align_batch(Q, T, idx[pick], idx[pick], opens[pick], **kw)
    _same([x[pick] for x in a], o, "align_skew 1 / oracle")


def _edge_call(rng, tlen, nfill=4100):
    """a call whose longest target has tlen bases: the longest query as a perfect match at the END of that target (highest score, in the cell with the largest frame),
    an unrelated pair (lowest score), a long overhang (half the query matches the start of the target), and short pairs that fill the batch up to the paired path"""
    q = LET[rng.integers(0, 4, 896)]
    ts = [np.concatenate([LET[rng.integers(0, 4, tlen - 896)], q]), LET[rng.integers(0, 4, tlen)], np.concatenate([q[:448], LET[rng.integers(0, 4, tlen - 448)]])]
    qs = [q, q, q]
    base = LET[rng.integers(0, 4, 330)]
    for _ in range(nfill):
        n = int(rng.integers(257, 320)); qs.append(_fit(rng, _mutate(rng, base, 0.1), n)); ts.append(_mutate(rng, base, 0.05))
    return _readset(qs), _readset(ts), np.arange(len(qs), dtype=np.uint32)


def test_range_edge_inside_outside_and_longest_target(gpu_api, oracle):
    """match 4, mismatch -8, open 16, ext 4: the longest target for which the host still runs the skewed instances, and one base more (the plain instances: the same
    results); ext 1 with a target of 4 000 bases, the longest of the 16-bit path.  The three special pairs of each call against the oracle, all pairs against align_skew 0"""
    rng = np.random.default_rng(52)
    t_in = max(t for t in range(896, 4001) if _span(4, 4, 16, 896, t) < 32768)
    assert _span(4, 4, 16, 896, t_in + 1) >= 32768 and _span(2, 1, 5, 896, 4000) < 32768
    for tlen, kw, open_ in ((t_in, dict(ext=4, match=4, mismatch=-8, k=13), 16), (t_in + 1, dict(ext=4, match=4, mismatch=-8, k=13), 16), (4000, dict(ext=1, match=2, mismatch=-2, k=13), 5)):
        Q, T, idx = _edge_call(rng, tlen)
        a, b, c = _three(gpu_api, Q, T, idx, idx, open_, **kw)
        _same(a, b, "target %d: align_skew 1 / 0" % tlen)
        _same(a, c, "target %d: align_skew 1 / align_paired 0" % tlen)
        sub = np.concatenate([np.arange(3), np.arange(3, len(idx), 97)])
        o = oracle.sg_align_batch(Q, T, idx[sub], idx[sub], open_, **kw)
        _same([x[sub] for x in a], o, "target %d: align_skew 1 / oracle" % tlen)
        assert a[0][0] == kw["match"] * 896


def test_skewed_spans_and_break_points(gpu_api):
    """aligned spans and per-window break points (the traceback walk: AlignJob.span / .bp) on a homopolymer-rich and a repeat-rich species: a polishing call with the
    affine read -> backbone aligner over > 4 096 reads returns the same sequences and counts with the skewed and the plain instances"""
    from ngspeciesid_amd._capi import polish_params
    rng = np.random.default_rng(53)
    species = [_homopolymers(rng, 720), _tandem(rng, 700)]
    reads = [_mutate(rng, sp, 0.08) for sp in species for _ in range(2100)]
    rs = _readset(reads)
    order = np.arange(len(reads), dtype=np.uint32)
    bb = ReadSet.from_strings([reads[0].tobytes().decode(), reads[2100].tobytes().decode()])
    res = {}
    try:
        for v in (1, 0):
            _opt(gpu_api, b"align_skew", v)
            res[v] = gpu_api.polish(bb, rs, [0, 2100, len(reads)], polish_params(iters=2, k=13, w=20, tile_depth=6, band=0, trim=2, aln_mode=0, stop_when_stable=0), read_order=order)
    finally:
        _opt(gpu_api, b"align_skew", 1)
    assert res[1][0] == res[0][0] and np.array_equal(res[1][1], res[0][1])
