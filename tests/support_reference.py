"""The definition of ngsid_consensus_support (include/ngsid_support.h) restated from the CPU oracle's parts.  Test infrastructure - never imported by the product.

Strand of a read: record [0] of the oracle's polish_trace(aln=True) with iters = 1 (the polisher's shared-minimizer rule).  Alignment columns: ongsid_i_ed_ops, an external
symbol of libngsid_oracle.so, through ctypes (0 '=', 1 'X', 2 'I' read only, 3 'D' centre only, forward order, the free centre ends as 'D').  Counting: numpy, here.
With source=columns_reference (tests/columns_reference.py) strands and columns come from the independent anchors instead, and no oracle is needed."""
import ctypes as C
import numpy as np
from ngspeciesid_amd._capi import ReadSet, polish_params

_COMP = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b
CLIP_RUN = 15


def ed_ops(oracle, read: np.ndarray, centre: np.ndarray) -> np.ndarray:
    f = oracle.lib.ongsid_i_ed_ops; f.restype = C.c_int
    read = np.ascontiguousarray(read, dtype=np.uint8); centre = np.ascontiguousarray(centre, dtype=np.uint8)
    ops = np.zeros(len(read) + len(centre) + 2, dtype=np.uint8)
    c = f(read.ctypes.data_as(C.c_void_p), C.c_int(len(read)), centre.ctypes.data_as(C.c_void_p), C.c_int(len(centre)), ops.ctypes.data_as(C.c_void_p))
    return ops[:c]


def strands(oracle, centres, rs, grp_off, read_order, k, w):
    """record [0] of every listed read.  error_threshold -1 makes the oracle's polisher drop every layer AFTER it has written the read's record, so the call costs the alignments
    only (no window graphs); the strand does not depend on it."""
    prm = polish_params(iters=1, k=k, w=w, aln_mode=1, error_threshold=-1.0)
    _, _, aln = oracle.polish_trace(ReadSet.from_strings(list(centres)), rs, grp_off, prm, read_order=read_order, aln=True)
    return np.asarray(aln)[0][:, 0].astype(np.int8)


def columns(oracle, source, read, centre):
    """the column list of one oriented read: the oracle's (source None), or source.ed_ops(read, centre) - tests/columns_reference.py, which needs no oracle"""
    return ed_ops(oracle, read, centre) if source is None else source.ed_ops(read, centre)


def strand_list(oracle, source, centres, rs, grp_off, read_order, k, w):
    return strands(oracle, centres, rs, grp_off, read_order, k, w) if source is None else source.strands(centres, rs, grp_off, read_order, k, w)


def count_read(oracle, cnt, read, centre, clip, source=None):
    """adds the counted columns of one oriented read to cnt [len(centre), 8]; -> True when the read counted at least one column"""
    ops = columns(oracle, source, read, centre)
    if clip:
        eq = np.concatenate(([0], (ops == 0).astype(np.int8), [0])); d = np.diff(eq)
        beg = np.nonzero(d == 1)[0]; end = np.nonzero(d == -1)[0] - 1          # runs of '=' columns [beg, end]
        ok = (end - beg + 1) >= CLIP_RUN
        if not ok.any(): return False
        x0, x1 = int(beg[ok][0]), int(end[ok][-1])
    else:
        dg = np.nonzero(ops <= 1)[0]
        if len(dg) == 0: return False
        x0, x1 = int(dg[0]), int(dg[-1])
    in_q = ops != 3; in_t = ops != 2
    qi = np.cumsum(in_q) - in_q; ti = np.cumsum(in_t) - in_t                    # read / centre position of every column (for a gap column: of the next base)
    o, q, t = ops[x0:x1 + 1], qi[x0:x1 + 1], ti[x0:x1 + 1]
    cnt[t[o != 2], 0] += 1
    cnt[t[o == 0], 1] += 1
    xs = o == 1; rb = read[q[xs]] & 0xDF                                        # upper case
    for c, letter in enumerate(b"ACGT"):
        cnt[t[xs][rb == letter], 2 + c] += 1
    cnt[t[o == 3], 6] += 1
    first_i = (o == 2) & (np.concatenate(([0], o[:-1])) != 2)                   # first column of every run of 'I' (x0 is never one)
    cnt[t[first_i] - 1, 7] += 1
    return True


def _part(oracle, centre_str, rs, reads, k, w, clip, source=None):
    """strands and counters of the listed reads `reads` (one group) against one centre"""
    st = strand_list(oracle, source, [centre_str], rs, np.array([0, len(reads)], dtype=np.uint64), reads, k, w)
    centre = np.frombuffer(centre_str.encode(), dtype=np.uint8); cnt = np.zeros((len(centre), 8), dtype=np.uint32); used = 0
    off = rs.off
    for x, r in enumerate(reads.tolist()):
        if st[x] < 0: continue
        read = rs.seq[int(off[r]):int(off[r + 1])]
        if st[x] == 1: read = _COMP[read[::-1]]
        used += count_read(oracle, cnt, np.ascontiguousarray(read), centre, clip, source)
    return st, cnt, used


def support_reference(oracle, centres, rs, grp_off, read_order=None, k=13, w=20, clip=False, threads=16, chunk=128, source=None):
    """-> (counts [total, 8] uint32, cen_off, n_used, strand) as Api.consensus_support returns them.  A read's strand and columns depend on its own centre only, so the listed
    reads are dealt to host threads in chunks (the oracle's C code runs outside the interpreter lock) and the counters summed.  source: where strands and columns come from -
    None: the oracle; tests/columns_reference.py: the independent anchor (oracle may then be None)."""
    from concurrent.futures import ThreadPoolExecutor
    grp_off = np.asarray(grp_off, dtype=np.uint64); ng = len(grp_off) - 1; nl = int(grp_off[-1])
    ro = np.arange(nl, dtype=np.uint32) if read_order is None else np.ascontiguousarray(read_order, dtype=np.uint32)
    cen_off = np.zeros(ng + 1, dtype=np.uint64); cen_off[1:] = np.cumsum([len(c) for c in centres])
    counts = np.zeros((int(cen_off[-1]), 8), dtype=np.uint32); used = np.zeros(ng, dtype=np.uint64); strand = np.full(nl, -1, dtype=np.int8)
    tasks = [(g, a, min(a + chunk, int(grp_off[g + 1]))) for g in range(ng) for a in range(int(grp_off[g]), int(grp_off[g + 1]), chunk)]
    with ThreadPoolExecutor(max_workers=threads) as ex:
        parts = list(ex.map(lambda t: _part(oracle, centres[t[0]], rs, ro[t[1]:t[2]].copy(), k, w, clip, source), tasks))
    for (g, a, b), (st, cnt, u) in zip(tasks, parts):
        strand[a:b] = st; counts[int(cen_off[g]):int(cen_off[g + 1])] += cnt; used[g] += u
    return counts, cen_off, used, strand
