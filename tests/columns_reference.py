"""An oracle-free source of what the store pass (ngsid_rec_walk) hands to its five consumers - the strand of every listed read and the forward column list of
every oriented (read, centre) pair - numpy and the standard library only.  Test infrastructure - never imported by the product.

It stands on the two anchors that share no code with oracle/ or the library: ed_reference.py (the ngsid_ed_align_batch contract: unit costs, free centre ends,
leftmost end column, traceback diagonal first, then read-only, then centre-only) and polish_reference.py (the polisher's strand rule of include/ngsid.h).  The
references of the consumers (support_, phase_, hp_, cigar_, errprof_reference.py) take this module as `source=` and then need no oracle at all; the oracle's
ongsid_i_ed_ops and strands are compared with it on the CPU (test_rec_reference_cpu.py), which hands the anchor to every oracle-based test as well.

Column codes as the oracle's: 0 '=' (both letters A/C/G/T in either case, and equal), 1 'X' (any other diagonal column), 2 'I' (read only), 3 'D' (centre only).
"""
import numpy as np
import ed_reference as ed
from polish_reference import minimizers, strand_call, revcomp

EQ, X, I, D = 0, 1, 2, 3
_ACGT = set("ACGTacgt")
_ops = {}
_mz = {}
_st = {}


def _text(s):
    if isinstance(s, str): return s
    return bytes(np.ascontiguousarray(s, dtype=np.uint8)).decode("latin-1")


def ops_of_path(read, centre, cols):
    """the forward column list of ONE path given by its diagonal columns [(read position, centre position)] in ascending order.  In front of the first diagonal column:
    the free centre prefix as 'D', then the read letters in front of it as 'I'; between two diagonal columns the centre-only columns, then the read-only ones (an
    optimal path holds only one of the two kinds there: a gap of each kind side by side costs 2 where one diagonal column costs at most 1); behind the last diagonal
    column the rest of the read as 'I', then the free centre suffix as 'D'.  A path without a diagonal column (every read letter read-only in front of the end
    column) is built by ed_ops."""
    n, m = len(read), len(centre)
    out = []
    pq, pt = -1, -1
    for k, (qi, ti) in enumerate(cols):
        qi, ti = int(qi), int(ti)
        dq, dt = qi - pq - 1, ti - pt - 1
        if k: assert not (dq and dt), ("an I run touches a D run inside the span", read, centre, qi, ti)
        out += [D] * dt + [I] * dq
        out.append(EQ if (read[qi] in _ACGT and centre[ti] in _ACGT and read[qi].upper() == centre[ti].upper()) else X)
        pq, pt = qi, ti
    out += [I] * (n - 1 - pq) + [D] * (m - 1 - pt)
    return np.array(out, dtype=np.uint8)


def ed_ops(read, centre):
    """the forward column list (uint8) of the oriented read against the centre, the free centre prefix and suffix as 'D'; strings, bytes or uint8 arrays"""
    read, centre = _text(read), _text(centre)
    key = (read, centre)
    if key not in _ops:
        if len(read) == 0:
            ops = np.full(len(centre), D, dtype=np.uint8)
        else:
            _, end, cols = ed.align_pair(read, centre)
            if len(cols): ops = ops_of_path(read, centre, cols)
            else: ops = np.array([D] * end + [I] * len(read) + [D] * (len(centre) - end), dtype=np.uint8)      # every read letter read-only at the end column
        assert int((ops != D).sum()) == len(read) and int((ops != I).sum()) == len(centre)
        ops.setflags(write=False)
        _ops[key] = ops
    return _ops[key]


def _sets(centre, k, w):
    key = (centre, k, w)
    if key not in _mz: _mz[key] = (frozenset(minimizers(centre, k, w)), frozenset(minimizers(revcomp(centre), k, w)))
    return _mz[key]


def strands(centres, rs, grp_off, read_order, k, w):
    """int8 per listed read: 0 plus, 1 minus, -1 no minimizer shared with its centre or the centre's reverse complement (include/ngsid.h, 'strand': the scheme is
    k' = min(k, 21), w' = max(w, k'))"""
    sk = min(k, 21); sw = max(w, sk)
    grp_off = np.asarray(grp_off, dtype=np.uint64); nl = int(grp_off[-1])
    ro = np.arange(nl, dtype=np.uint32) if read_order is None else np.asarray(read_order)
    out = np.full(nl, -1, dtype=np.int8)
    for g in range(len(grp_off) - 1):
        centre = _text(centres[g])
        fwd, rev = _sets(centre, sk, sw)
        for x in range(int(grp_off[g]), int(grp_off[g + 1])):
            r = int(ro[x]); read = _text(rs.seq[int(rs.off[r]):int(rs.off[r + 1])])
            key = (read, centre, sk, sw)
            if key not in _st: _st[key] = strand_call(read, fwd, rev, sk, sw)[2]
            out[x] = _st[key]
    return out


def oriented(read, strand):
    """the read as the aligner sees it: as listed on the plus strand, its reverse complement (A<->T, C<->G, anything else N) on the minus strand"""
    read = _text(read)
    return revcomp(read) if strand == 1 else read
