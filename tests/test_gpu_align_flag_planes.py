"""The traceback flags of the paired int16 aligner (csrc/k_align16p.hip) are stored as bit planes: byte f of the 32-bit half k of a traceback word holds flag f
of rows 8 k .. 8 k + 7 of a lane, one bit per row, and the row state is g = H - open.  These tests aim at that layout: query lengths on every residue
(n - 1) mod R of the four length classes (rows 8 - 13 of a lane live in the second half of the word), bins of odd size (items with one pair), homopolymer and
tandem-repeat pairs (ties of the diagonal against a gap, of E against F and of open against extend) and a different gap open per pair of an item.
The paired kernel must return what the one-pair kernel (ngsid_ctx_option align_paired = 0) and the oracle return.
"""
import ctypes as C
import numpy as np
import pytest
from ngspeciesid_amd._capi import ReadSet

pytestmark = pytest.mark.gpu
LET = np.frombuffer(b"ACGT", dtype=np.uint8)
NAMES = ("score", "ncols", "nmatch", "region")
CLASSES = ((4, 200, 256), (8, 400, 512), (12, 700, 768), (14, 790, 896))     # rows per lane, lowest and highest query length used in the class


def _opt(api, name, v):
    assert api.lib.ngsid_ctx_option(api.ctx, name, C.c_int64(v)) == 0


def _mutate(rng, s, rate):
    out = []
    for c in s:
        u = rng.random()
        if u < rate * 0.4: out.append(int(LET[rng.integers(0, 4)]))
        elif u < rate * 0.7: continue
        elif u < rate: out.append(int(c)); out.append(int(LET[rng.integers(0, 4)]))
        else: out.append(int(c))
    return np.array(out, dtype=np.uint8)


def _homopolymers(rng, n):
    runs = []
    while sum(len(r) for r in runs) < n:
        runs.append(np.full(int(rng.integers(1, 12)), LET[rng.integers(0, 4)], dtype=np.uint8))
    return np.concatenate(runs)[:n]


def _tandem(rng, n):
    unit = LET[rng.integers(0, 4, int(rng.integers(1, 7)))]
    return np.tile(unit, n // len(unit) + 1)[:n]


def _fit(rng, q, n):
    """q cut or padded (with its own letters) to exactly n bases"""
    if len(q) >= n: return q[:n]
    return np.concatenate([q, q[rng.integers(0, len(q), n - len(q))]])


def _batch(seed):
    """> 4 096 pairs (the paired path) whose query lengths cover every residue of every class; each residue gets an odd or an even number of pairs"""
    rng = np.random.default_rng(seed)
    qs, ts = [], []
    for R, lo, hi in CLASSES:
        for res in range(R):
            n_first = lo + ((res - (lo - 1)) % R)                               # the first length >= lo with (n - 1) mod R == res
            lens = np.arange(n_first, hi + 1, R)
            for rep in range(int(rng.integers(40, 70)) * 2 + (res & 1)):        # odd counts on odd residues: a bin whose last item holds one pair
                n = int(lens[rep % len(lens)]) if rep < len(lens) else int(rng.choice(lens))
                kind = rng.random()
                if kind < 0.3: base = _homopolymers(rng, n + 40)
                elif kind < 0.6: base = _tandem(rng, n + 40)
                else: base = LET[rng.integers(0, 4, n + 40)]
                t = _mutate(rng, base, float(rng.choice([0.0, 0.03, 0.12])))
                q = _fit(rng, _mutate(rng, base, float(rng.choice([0.0, 0.05, 0.15]))), n)
                if rng.random() < 0.15: t = t[int(rng.integers(0, 60)):]           # overhangs on either side
                if rng.random() < 0.15: q = _fit(rng, q[int(rng.integers(0, 40)):], n)
                if rng.random() < 0.05: q = q.copy(); q[rng.integers(0, n, 2)] = ord("N")
                qs.append(q); ts.append(t)
    while len(qs) < 4200:                                                          # fill up to the paired path's batch size (one class-2 residue grows)
        n = 713; base = _tandem(rng, n + 20); qs.append(_fit(rng, _mutate(rng, base, 0.05), n)); ts.append(_mutate(rng, base, 0.05))
    Q = ReadSet(np.concatenate(qs), None, np.concatenate(([0], np.cumsum([len(x) for x in qs]))).astype(np.uint64))
    T = ReadSet(np.concatenate(ts), None, np.concatenate(([0], np.cumsum([len(x) for x in ts]))).astype(np.uint64))
    idx = np.arange(len(qs), dtype=np.uint32)
    return rng, Q, T, idx, np.array([len(q) for q in qs])


def _both(api, Q, T, idx, opens, **kw):
    try:
        _opt(api, b"align_paired", 1); a = api.sg_align_batch(Q, T, idx, idx, opens, **kw)
        _opt(api, b"align_paired", 0); b = api.sg_align_batch(Q, T, idx, idx, opens, **kw)
    finally:
        _opt(api, b"align_paired", 1)
    return a, b


@pytest.mark.parametrize("seed,ext,match,mismatch,olo,ohi", [(41, 1, 2, -2, 1, 6), (42, 4, 4, -8, 4, 17)])
def test_flag_planes_every_residue(gpu_api, oracle, seed, ext, match, mismatch, olo, ohi):
    """every residue of every class, per-pair open (open == ext in part of the pairs of the first case), against the one-pair kernel and the oracle"""
    rng, Q, T, idx, qlen = _batch(seed)
    opens = rng.integers(olo, ohi, len(idx)).astype(np.int32)
    kw = dict(ext=ext, match=match, mismatch=mismatch, k=13)
    a, b = _both(gpu_api, Q, T, idx, opens, **kw)
    for x, y, nm in zip(a, b, NAMES):
        bad = np.nonzero(x != y)[0]
        assert len(bad) == 0, "%s: paired != one-pair kernel at pairs %s (query lengths %s)" % (nm, bad[:8].tolist(), qlen[bad[:8]].tolist())
    # the oracle on a subset that holds the last residue(s) of each class: rows 8 - 13 of a lane for R = 12 / 14
    pick = []
    for R, lo, hi in CLASSES:
        cls = np.nonzero((qlen >= lo) & (qlen <= hi))[0]
        for res in sorted({0, R - 1, R // 2, 8 % R, (9 % R)}):
            sel = cls[(qlen[cls] - 1) % R == res]
            pick.extend(sel[:6].tolist())
    pick = np.array(sorted(set(pick)), dtype=np.int64)
    o = oracle.sg_align_batch(Q, T, idx[pick], idx[pick], opens[pick], **kw)
    for x, y, nm in zip(a, o, NAMES):
        bad = np.nonzero(x[pick] != y)[0]
        assert len(bad) == 0, "%s: paired != oracle at pairs %s" % (nm, pick[bad[:8]].tolist())


def test_flag_planes_spans_and_break_points(gpu_api):
    """aligned spans and the per-window break points (the traceback walk of the paired kernel, AlignJob.span / .bp) on homopolymer- and repeat-rich
    species: a polishing call with the affine read -> backbone aligner over > 4 096 reads returns the same sequences and counts with either kernel"""
    from ngspeciesid_amd._capi import polish_params
    rng = np.random.default_rng(7)
    species = [_homopolymers(rng, 720), _tandem(rng, 700)]
    reads = []
    for sp in species:
        for _ in range(2100):
            reads.append(_mutate(rng, sp, 0.08))
    rs = ReadSet(np.concatenate(reads), None, np.concatenate(([0], np.cumsum([len(x) for x in reads]))).astype(np.uint64))
    order = np.arange(len(reads), dtype=np.uint32)
    bb = ReadSet.from_strings([reads[0].tobytes().decode(), reads[2100].tobytes().decode()])
    res = {}
    try:
        for v in (1, 0):
            _opt(gpu_api, b"align_paired", v)
            res[v] = gpu_api.polish(bb, rs, [0, 2100, len(reads)], polish_params(iters=2, k=13, w=20, tile_depth=6, band=0, trim=2, aln_mode=0, stop_when_stable=0), read_order=order)
    finally:
        _opt(gpu_api, b"align_paired", 1)
    assert res[1][0] == res[0][0] and np.array_equal(res[1][1], res[0][1])
