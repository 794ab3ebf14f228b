"""The definition of ngsid_hp_runs (include/ngsid_hp.h) restated from the CPU oracle's parts in plain numpy.  Test infrastructure - never imported by the product.

Strands and alignment columns: tests/support_reference.py (record [0] of the oracle's polish trace; ongsid_i_ed_ops: 0 '=', 1 'X', 2 'I' read only, 3 'D' centre only).
Read and centre position of every column: cumulative sums, as count_read does.  The histogram: here."""
import numpy as np
from support_reference import strands, ed_ops, columns, strand_list, _COMP, CLIP_RUN

NBUCKET, OTHER = 17, 16


def run_end(centre, a):
    b = a + 1
    while b < len(centre) and centre[b] == centre[a]: b += 1
    return b


def read_runs(ops, read, centre, starts, clip):
    """ops: the columns of ONE oriented read against centre -> bucket per listed run (-1: the read adds nothing)"""
    out = np.full(len(starts), -1, dtype=np.int64)
    ops = np.asarray(ops, dtype=np.uint8)
    if clip:
        eq = np.concatenate(([0], (ops == 0).astype(np.int8), [0])); d = np.diff(eq)
        beg = np.nonzero(d == 1)[0]; end = np.nonzero(d == -1)[0] - 1
        ok = (end - beg + 1) >= CLIP_RUN
        if not ok.any(): return out
        x0, x1 = int(beg[ok][0]), int(end[ok][-1])
    else:
        dg = np.nonzero(ops <= 1)[0]
        if len(dg) == 0: return out
        x0, x1 = int(dg[0]), int(dg[-1])
    in_q = ops != 3; in_t = ops != 2
    qi = np.cumsum(in_q) - in_q; ti = np.cumsum(in_t) - in_t
    t_begin, t_end = int(ti[x0]), int(ti[x1])
    col_of = {int(ti[x]): x for x in range(len(ops)) if ops[x] != 2}          # the column that consumes every centre position
    m = len(centre)
    for j, a in enumerate(int(s) for s in starts):
        b = run_end(centre, a); c = centre[a] & 0xDF
        if c not in b"ACGT": continue
        if not (a >= 1 and b <= m - 1 and t_begin <= a - 1 and b <= t_end): continue
        xa, xb = col_of[a - 1], col_of[b]
        if ops[xa] != 0 or ops[xb] != 0:
            out[j] = OTHER; continue
        qa, qb = int(qi[xa]), int(qi[xb])
        between = read[qa + 1:qb] & 0xDF
        out[j] = min(qb - qa - 1, 15) if (between == c).all() else OTHER
    return out


def check_lists(centres, run_off, run_start):
    """the argument errors of the call -> True when the lists are legal"""
    for g, cs in enumerate(centres):
        c = cs.encode(); prev = -1
        for a in (int(x) for x in run_start[int(run_off[g]):int(run_off[g + 1])]):
            if a >= len(c) or a <= prev or (a > 0 and c[a - 1] == c[a]): return False
            prev = a
    return True


def hp_reference(oracle, centres, rs, grp_off, run_off, run_start, read_order=None, k=13, w=20, clip=False, source=None):
    """-> (hist [n_runs, 2, 17] uint32, strand) as Api.hp_runs returns them; source as in support_reference"""
    grp_off = np.asarray(grp_off, dtype=np.uint64); run_off = np.asarray(run_off, dtype=np.uint64); run_start = np.asarray(run_start, dtype=np.uint32)
    assert check_lists(centres, run_off, run_start)
    ng = len(grp_off) - 1; nl = int(grp_off[-1])
    ro = np.arange(nl, dtype=np.uint32) if read_order is None else np.ascontiguousarray(read_order, dtype=np.uint32)
    hist = np.zeros((int(run_off[-1]), 2, NBUCKET), dtype=np.uint32); strand = np.full(nl, -1, dtype=np.int8)
    for g in range(ng):
        a, b = int(grp_off[g]), int(grp_off[g + 1])
        if a == b: continue
        st = strand_list(oracle, source, [centres[g]], rs, np.array([0, b - a], dtype=np.uint64), ro[a:b].copy(), k, w)
        strand[a:b] = st
        starts = run_start[int(run_off[g]):int(run_off[g + 1])]
        if len(starts) == 0: continue
        centre = np.frombuffer(centres[g].encode(), dtype=np.uint8)
        for x, r in enumerate(ro[a:b].tolist()):
            if st[x] < 0: continue
            read = rs.seq[int(rs.off[r]):int(rs.off[r + 1])]
            if st[x] == 1: read = _COMP[read[::-1]]
            read = np.ascontiguousarray(read)
            bk = read_runs(columns(oracle, source, read, centre), read, centre, starts, clip)
            for j in np.nonzero(bk >= 0)[0]:
                hist[int(run_off[g]) + j, int(st[x]), bk[j]] += 1
    return hist, strand


class HpAdapter:
    """an oracle-backed Api whose hp_runs is answered by the reference definition; everything else is the oracle's"""
    def __init__(self, oracle):
        self._o = oracle

    def __getattr__(self, name):
        return getattr(self._o, name)

    def hp_runs(self, centres, rs, grp_off, run_off, run_start, read_order=None, k=13, w=20, clip=False):
        return hp_reference(self._o, [centres.get(i)[0] for i in range(centres.n)], rs, grp_off, run_off, run_start, read_order, k, w, clip)
