"""The definition of ngsid_read_cigars (include/ngsid_cigar.h) restated from the CPU oracle's parts.  Test infrastructure - never imported by the product.

Strands and alignment columns as tests/support_reference.py (the oracle's polish_trace record [0], ongsid_i_ed_ops); the counted columns, the spans, nm and the run
lengths in numpy, here.  cigar_reference returns exactly what Api.read_cigars returns."""
import numpy as np
from support_reference import ed_ops, strands, columns, strand_list, _COMP, CLIP_RUN

OP_M, OP_I, OP_D, OP_S, OP_EQ, OP_X = 0, 1, 2, 4, 7, 8
COLUMN_OP = np.array([OP_EQ, OP_X, OP_I, OP_D], dtype=np.int64)                 # the oracle's column codes 0 '=' 1 'X' 2 'I' 3 'D' as BAM ops


def counted(ops, clip):
    """(x0, x1): the first and the last counted column of a column list, or None"""
    if clip:
        eq = np.concatenate(([0], (ops == 0).astype(np.int8), [0])); d = np.diff(eq)
        beg = np.nonzero(d == 1)[0]; end = np.nonzero(d == -1)[0] - 1
        ok = (end - beg + 1) >= CLIP_RUN
        if not ok.any(): return None
        return int(beg[ok][0]), int(end[ok][-1])
    dg = np.nonzero(ops <= 1)[0]
    if len(dg) == 0: return None
    return int(dg[0]), int(dg[-1])


def rle(codes):
    """run-length encoding of a list of BAM op codes -> [(length, op)]"""
    codes = np.asarray(codes, dtype=np.int64)
    if len(codes) == 0: return []
    cut = np.concatenate(([0], np.nonzero(np.diff(codes))[0] + 1, [len(codes)]))
    return [(int(b - a), int(codes[a])) for a, b in zip(cut[:-1], cut[1:])]


def cigar_of_columns(ops, L, clip, merge_m=False):
    """one oriented read of L letters, its forward column list -> (aln [5] or None, [(length, op)])"""
    c = counted(ops, clip)
    if c is None: return None, []
    x0, x1 = c
    in_q = ops != 3; in_t = ops != 2
    qi = np.cumsum(in_q) - in_q; ti = np.cumsum(in_t) - in_t
    o = ops[x0:x1 + 1]
    qb, qe, tb, te = int(qi[x0]), int(qi[x1]), int(ti[x0]), int(ti[x1])
    codes = COLUMN_OP[o]
    if merge_m: codes = np.where((codes == OP_EQ) | (codes == OP_X), OP_M, codes)
    runs = ([(qb, OP_S)] if qb else []) + rle(codes) + ([(L - 1 - qe, OP_S)] if L - 1 - qe else [])
    return [tb, te, qb, qe, int((o != 0).sum())], runs


def walk_record(cigar, seq, target, pos):
    """walks the ops [(length, letter)] of one SAM record over its SEQ and the target from the 1-based POS: asserts that '=' columns hold equal ACGT letters, 'X' columns
    do not, and that the read is consumed exactly -> (nm, target letters consumed)"""
    qi, ti, nm = 0, pos - 1, 0
    for n, op in cigar:
        assert n > 0
        if op in "=X":
            for d in range(n):
                a, b = seq[qi + d].upper(), target[ti + d].upper()
                assert (a == b and a in "ACGT") == (op == "="), (op, qi + d, ti + d, a, b)
        if op in "XID": nm += n
        if op == "M": nm += sum(not (seq[qi + d].upper() == target[ti + d].upper() and seq[qi + d].upper() in "ACGT") for d in range(n))
        if op in "M=XIS": qi += n
        if op in "M=XD": ti += n
    assert qi == len(seq) and ti <= len(target)
    return nm, ti - (pos - 1)


def oriented(rs, r, strand):
    read = rs.seq[int(rs.off[r]):int(rs.off[r + 1])]
    return np.ascontiguousarray(_COMP[read[::-1]] if strand == 1 else read)


def cigar_reference(oracle, centres, rs, grp_off, read_order=None, k=13, w=20, clip=False, merge_m=False, only=None, source=None):
    """-> (aln [n_listed, 5] int32, op_off [n_listed + 1] uint64, ops uint32, strand [n_listed] int8) as Api.read_cigars returns them.  only: a set of listed positions -
    the others get no ops and -1 (for a sample of a large call; their strand is still filled); source as in support_reference"""
    grp_off = np.asarray(grp_off, dtype=np.uint64); ng = len(grp_off) - 1; nl = int(grp_off[-1])
    ro = np.arange(nl, dtype=np.uint32) if read_order is None else np.ascontiguousarray(read_order, dtype=np.uint32)
    st = strand_list(oracle, source, centres, rs, grp_off, ro, k, w) if nl else np.zeros(0, np.int8)
    aln = np.full((nl, 5), -1, dtype=np.int32); op_off = np.zeros(nl + 1, dtype=np.uint64); ops = []
    for g in range(ng):
        centre = np.frombuffer(centres[g].encode(), dtype=np.uint8)
        for x in range(int(grp_off[g]), int(grp_off[g + 1])):
            op_off[x + 1] = op_off[x]
            if st[x] < 0 or (only is not None and x not in only) or len(centre) == 0: continue
            read = oriented(rs, int(ro[x]), int(st[x]))
            a, runs = cigar_of_columns(columns(oracle, source, read, centre), len(read), clip, merge_m)
            if a is None: continue
            aln[x] = a; ops += [(l << 4) | o for l, o in runs]; op_off[x + 1] = op_off[x] + np.uint64(len(runs))
    return aln, op_off, np.array(ops, dtype=np.uint32), st
