"""The step logic of k_errprof (csrc/k_errprof.hip) in Python integers.  Test infrastructure - never imported by the product.

walk(): one wave on one pair - aligned steps of 64 centre positions; class, flag and centre byte of the position before come from the lane below and, for lane 0, from the
last position of the step before; a 'D' run is found with one 64-bit mask per step and the run that reaches lane 63 is carried as a length; an 'I' run is counted by the lane
BEHIND it from the two read positions around it.  The rows are those of tests/cigar_wave_model.py (rows_of_columns): cells the aligner leaves unwritten hold GARBAGE, so a
walk that reads one is found out."""
import numpy as np
from cigar_wave_model import REC_EQ, REC_SUB, REC_OTHER, REC_DEL, GARBAGE_NIB, GARBAGE_POS, MASK64, _code

NCOUNT, NQ = 96, 94
PAIR, INS_LETTER, CEN_OTHER, READS, INS_LEN, DEL_LEN, HPCTX = 0, 24, 29, 30, 32, 48, 64


def centre_bytes(centre):
    """per centre position min(run length, 8) | letter code << 4 (the host side of ngsid_error_profile)"""
    c = [int(v) for v in centre]; out = [0] * len(c); a = 0
    while a < len(c):
        b = a + 1
        while b < len(c) and c[b] == c[a]: b += 1
        for i in range(a, b): out[i] = min(b - a, 8) | (_code(c[a]) << 4)
        a = b
    return out


def _q(byte): return min(max(int(byte) - 33, 0), NQ - 1)
def _len(l): return min(l, 16) - 1


def walk(nib, pos, span, read, qual, centre):
    """one wave: -> (cnt [96], qt [94][3]) of the pair with span = (q_begin, q_end, t_begin, t_end); qual None: qt stays zero"""
    cnt = [0] * NCOUNT; qt = [[0, 0, 0] for _ in range(NQ)]
    qb, qe, tb, te = span; L = len(read); m = len(centre)
    if tb < 0 or te < tb or te >= m or qb < 0 or qe < qb or qe >= L: return cnt, qt
    cx = centre_bytes(centre)
    cnt[READS] += 1
    carry_del = carry_flag = carry_ctx = 0; d_open = 0
    for base in range(tb & ~63, te + 1, 64):
        valid = [tb <= base + l <= te for l in range(64)]
        nb = [int(nib[base + l]) if valid[l] else 0 for l in range(64)]
        for l in range(64):
            assert not valid[l] or nb[l] != GARBAGE_NIB, "unwritten nibble read at %d" % (base + l)
        code = [v & 7 for v in nb]; flag = [v >> 3 for v in nb]
        ctx = [cx[base + l] if valid[l] else 0 for l in range(64)]
        is_eq = [valid[l] and code[l] == REC_EQ for l in range(64)]; is_del = [valid[l] and code[l] == REC_DEL for l in range(64)]
        is_x = [valid[l] and REC_SUB <= code[l] <= REC_OTHER for l in range(64)]
        pd = [carry_del] + [int(v) for v in is_del[:63]]; pf = [carry_flag] + flag[:63]; pctx = [carry_ctx] + ctx[:63]
        insb = [valid[l] and base + l > tb and pf[l] == 1 and not pd[l] and not is_del[l] for l in range(64)]
        D = sum(1 << l for l in range(64) if is_del[l])
        if d_open and not (D & 1): cnt[DEL_LEN + _len(d_open)] += 1
        for l in range(64):
            b = base + l; cc = ctx[l] >> 4; rl = (ctx[l] & 15) - 1
            if is_eq[l] and cc < 4:
                cnt[PAIR + cc * 7] += 1; cnt[HPCTX + rl * 4] += 1
            if qual is not None and (is_eq[l] or is_x[l]):
                x = int(pos[b]); assert x != GARBAGE_POS, "position read at a cell that holds none"
                if x < L: qt[_q(qual[x])][0 if is_eq[l] else 1] += 1
            if is_x[l] or is_del[l]:
                o = 5 if is_del[l] else code[l] - REC_SUB
                if cc < 4:
                    cnt[PAIR + cc * 6 + o] += 1; cnt[HPCTX + rl * 4 + (2 if is_del[l] else 1)] += 1
                else: cnt[CEN_OTHER] += 1
            if is_del[l] and l < 63 and not (D >> (l + 1)) & 1:
                gap = ~D & ((1 << l) - 1)
                cnt[DEL_LEN + _len(l - (gap.bit_length() - 1) if gap else l + 1 + d_open)] += 1
            if insb[l]:
                qa, qz = int(pos[b - 1]), int(pos[b])
                assert qa != GARBAGE_POS and qz != GARBAGE_POS, "position read at a cell that holds none"
                if qa + 1 < qz < L:
                    cnt[INS_LEN + _len(qz - qa - 1)] += 1
                    if (pctx[l] >> 4) < 4 and pctx[l] & 15: cnt[HPCTX + ((pctx[l] & 15) - 1) * 4 + 3] += 1
                    for i in range(qa + 1, qz):
                        cnt[INS_LETTER + _code(int(read[i]))] += 1
                        if qual is not None: qt[_q(qual[i])][2] += 1
        if (D >> 63) & 1:
            nd = ~D & MASK64
            d_open = 64 - nd.bit_length() if nd else d_open + 64
        else: d_open = 0
        v1 = min(te - base, 63)
        carry_del, carry_flag, carry_ctx = int(is_del[v1]), flag[v1], ctx[v1]
    if d_open: cnt[DEL_LEN + _len(d_open)] += 1
    return cnt, qt
