"""The definition of ngsid_error_profile (include/ngsid_errprof.h) restated from the CPU oracle's parts.  Test infrastructure - never imported by the product.

Strands and alignment columns as tests/support_reference.py (the oracle's polish_trace record [0], ongsid_i_ed_ops), the counted columns as tests/cigar_reference.py; the
tables in numpy, here, from the column list, the oriented read, the oriented qualities and the centre.  errprof_reference returns exactly what Api.error_profile returns."""
import numpy as np
from support_reference import ed_ops, strands, columns, strand_list
from cigar_reference import counted, oriented

NCOUNT, NQ = 96, 94
PAIR, INS_LETTER, CEN_OTHER, READS, INS_LEN, DEL_LEN, HPCTX = 0, 24, 29, 30, 32, 48, 64
_CODE = np.full(256, 4, dtype=np.int64)
for _i, _l in enumerate("ACGT"):
    _CODE[ord(_l)] = _i; _CODE[ord(_l.lower())] = _i


def run_lengths(centre):
    """per position the length of the maximal run of equal bytes that holds it"""
    c = np.asarray(centre); out = np.zeros(len(c), dtype=np.int64)
    a = 0
    while a < len(c):
        b = a + 1
        while b < len(c) and c[b] == c[a]: b += 1
        out[a:b] = b - a; a = b
    return out


def _runs(mask):
    """lengths of the maximal runs of True"""
    d = np.diff(np.concatenate(([0], mask.astype(np.int8), [0])))
    return np.nonzero(d == -1)[0] - np.nonzero(d == 1)[0]


def profile_columns(cnt, qt, ops, read, qual, centre, clip):
    """adds one oriented read (its forward column list ops: 0 '=' 1 'X' 2 'I' 3 'D', its letters, its oriented quality bytes or None) to cnt [96] and qt [94, 3] (or None)"""
    c = counted(ops, clip)
    if c is None: return
    x0, x1 = c
    in_q = ops != 3; in_t = ops != 2
    qi = np.cumsum(in_q) - in_q; ti = np.cumsum(in_t) - in_t
    o, q, t = ops[x0:x1 + 1], qi[x0:x1 + 1], ti[x0:x1 + 1]
    read = np.asarray(read, dtype=np.uint8)
    add = lambda idx: np.bincount(np.asarray(idx, dtype=np.int64), minlength=NCOUNT).astype(np.uint64)
    cnt[READS] += np.uint64(1)
    ins = o == 2; col = ~ins                                                    # 'I' columns; the columns that consume a centre base
    cnt += add(INS_LETTER + _CODE[read[q[ins]]])
    c_ = _CODE[np.asarray(centre, dtype=np.uint8)][t[col]]                       # the centre letter of every such column, ...
    out = np.where(o[col] == 3, 5, _CODE[read[np.minimum(q[col], len(read) - 1)]])      # ... what it became, ...
    r = np.minimum(run_lengths(centre)[t[col]], 8) - 1                          # ... the run it sits in, ...
    kind = np.array([0, 1, 0, 2])[o[col]]                                       # ... '=' 'X' 'D', ...
    behind = np.concatenate((ins[1:], [False]))[col]                            # ... and whether an 'I' run follows it directly
    acgt = c_ < 4
    cnt += add(PAIR + c_[acgt] * 6 + out[acgt])
    cnt += add(HPCTX + r[acgt] * 4 + kind[acgt])
    cnt += add(HPCTX + r[acgt & behind] * 4 + 3)
    cnt[CEN_OTHER] += np.uint64(int((~acgt & (o[col] != 0)).sum()))
    cnt += add(INS_LEN + np.minimum(_runs(ins), 16) - 1)
    cnt += add(DEL_LEN + np.minimum(_runs(o == 3), 16) - 1)
    if qt is not None and qual is not None:
        rd = o != 3                                                             # the columns that hold a read base
        qq = np.clip(np.asarray(qual, dtype=np.int64)[q[rd]] - 33, 0, NQ - 1)
        qt += np.bincount(qq * 3 + np.array([0, 1, 2, 0])[o[rd]], minlength=NQ * 3).astype(np.uint64).reshape(NQ, 3)


def errprof_reference(oracle, centres, rs, grp_off, read_order=None, k=13, w=20, clip=False, qualities=True, source=None):
    """-> (counts [n_groups, 2, 96] uint64, qtab [n_groups, 2, 94, 3] uint64 or None, strand [n_listed] int8) as Api.error_profile returns them; source as in support_reference"""
    grp_off = np.asarray(grp_off, dtype=np.uint64); ng = len(grp_off) - 1; nl = int(grp_off[-1])
    ro = np.arange(nl, dtype=np.uint32) if read_order is None else np.ascontiguousarray(read_order, dtype=np.uint32)
    st = strand_list(oracle, source, centres, rs, grp_off, ro, k, w) if nl else np.zeros(0, np.int8)
    counts = np.zeros((ng, 2, NCOUNT), dtype=np.uint64); qtab = np.zeros((ng, 2, NQ, 3), dtype=np.uint64) if qualities else None
    for g in range(ng):
        centre = np.frombuffer(centres[g].encode(), dtype=np.uint8)
        for x in range(int(grp_off[g]), int(grp_off[g + 1])):
            if st[x] < 0 or len(centre) == 0: continue
            r = int(ro[x]); s = int(st[x])
            read = oriented(rs, r, s)
            qual = None
            if rs.qual is not None:
                qual = rs.qual[int(rs.off[r]):int(rs.off[r + 1])]
                if s == 1: qual = qual[::-1]
            profile_columns(counts[g, s], None if qtab is None else qtab[g, s], columns(oracle, source, read, centre), read, qual, centre, clip)
    return counts, qtab, st


def check_identities(counts, qtab, support, cen_off, used, aln, grp_off):
    """the identities of include/ngsid_errprof.h, group by group (centres of ACGT: CEN_OTHER has no 'D' part)"""
    for g in range(len(grp_off) - 1):
        c = counts[g].sum(axis=0).astype(np.int64); sup = support[int(cen_off[g]):int(cen_off[g + 1])].astype(np.int64).sum(axis=0)
        pair = c[PAIR:PAIR + 24].reshape(4, 6)
        assert pair.sum() + c[CEN_OTHER] == sup[0]                                # DEPTH
        assert np.trace(pair[:, :4]) == sup[1]                                    # AGREE
        assert pair[:, 5].sum() == sup[6] and c[CEN_OTHER] == 0                   # DEL
        assert c[INS_LEN:INS_LEN + 16].sum() == sup[7]                            # INS
        assert c[HPCTX:HPCTX + 32].reshape(8, 4)[:, :3].sum() == pair.sum()
        a = aln[int(grp_off[g]):int(grp_off[g + 1])]
        n_x = pair[:, :5].sum() - np.trace(pair[:, :4])
        assert n_x + c[INS_LETTER:INS_LETTER + 5].sum() + pair[:, 5].sum() == a[a[:, 0] >= 0, 4].sum()      # nm
        assert c[READS] == used[g] == (a[:, 0] >= 0).sum() and c[31] == 0
        assert c[DEL_LEN:DEL_LEN + 16].sum() <= pair[:, 5].sum()
        if qtab is not None:
            q = qtab[g].sum(axis=(0, 1)).astype(np.int64)
            assert q[0] == np.trace(pair[:, :4]) and q[2] == c[INS_LETTER:INS_LETTER + 5].sum() and q[1] == n_x
