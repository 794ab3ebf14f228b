"""The step logic of k_cigar_walk (csrc/k_cigar.hip) in Python integers, and the rows it reads.  Test infrastructure - never imported by the product.

walk(): one wave on one pair - aligned steps of 64 centre positions, a 64-bit run-start mask per step, an op's index by the popcount of the bits below its lane, a
run's length by the next set bit, the run open at the end of a step carried into the next.  rows_of_columns() writes the path nibbles and read positions of a forward
column list as the aligner records them; traceback_columns() is a small unit-cost aligner with the aligner's rules (read end to end, centre ends free, leftmost
minimum, diagonal before read-only before centre-only) for hand-made pairs.  Cells the aligner leaves unwritten hold GARBAGE here, so a walk that reads one is found out."""
import numpy as np

REC_EQ, REC_SUB, REC_OTHER, REC_DEL, REC_INS = 1, 2, 6, 7, 8
OP_M, OP_I, OP_D, OP_S, OP_EQ, OP_X = 0, 1, 2, 4, 7, 8
GARBAGE_NIB, GARBAGE_POS = 0xF, 0xFFFF
MASK64 = (1 << 64) - 1


def _code(c):
    return "ACGT".find(chr(c & 0xDF)) if chr(c & 0xDF) in "ACGT" else 4


def traceback_columns(read, centre):
    """forward column list (0 '=', 1 'X', 2 'I', 3 'D'; no columns for the free centre ends) and the centre position of its first column"""
    n, m = len(read), len(centre)
    q = [_code(c) for c in read]; t = [_code(c) for c in centre]
    D = np.zeros((n + 1, m + 1), dtype=np.int64); D[:, 0] = np.arange(n + 1)
    for i in range(1, n + 1):
        sub = D[i - 1, :-1] + np.array([0 if (q[i - 1] == tj and tj < 4) else 1 for tj in t], dtype=np.int64)
        row = np.minimum(sub, D[i - 1, 1:] + 1)
        for j in range(1, m + 1):                                            # the horizontal dependency
            D[i, j] = min(int(row[j - 1]), int(D[i, j - 1]) + 1)
    j = int(np.argmin(D[n])); i = n; cols = []
    while i > 0:
        if j > 0 and D[i, j] == D[i - 1, j - 1] + (0 if (q[i - 1] == t[j - 1] and q[i - 1] < 4) else 1):
            cols.append(0 if q[i - 1] == t[j - 1] and q[i - 1] < 4 else 1); i -= 1; j -= 1
        elif D[i, j] == D[i - 1, j] + 1 or j == 0:
            cols.append(2); i -= 1
        else:
            cols.append(3); j -= 1
    return np.array(cols[::-1], dtype=np.uint8), j


def rows_of_columns(cols, read, m, t0=0):
    """nibble row [m] and position row [m] of a forward column list whose first column lies at centre position t0 (the oracle's lists carry the free centre ends as
    'D' and start at 0).  Only the positions between the first and the last column that consumes a read letter are written; a 'D' position holds no read position."""
    nib = np.full(m, GARBAGE_NIB, dtype=np.int64); pos = np.full(m, GARBAGE_POS, dtype=np.int64)
    cols = np.asarray(cols); on = np.nonzero(cols != 3)[0]
    if len(on) == 0: return nib, pos
    qi, ti = 0, t0
    for x, c in enumerate(cols.tolist()):
        inside = on[0] <= x <= on[-1]
        if c == 2:
            if inside and ti > t0 and nib[ti - 1] != GARBAGE_NIB: nib[ti - 1] |= REC_INS
            qi += 1; continue
        if inside:
            if c == 3: nib[ti] = REC_DEL
            else:
                k = _code(int(read[qi]))
                nib[ti] = REC_EQ if c == 0 else (REC_SUB + k if k < 4 else REC_OTHER); pos[ti] = qi
        if c != 3: qi += 1
        ti += 1
    return nib, pos


def _popc(x): return bin(x).count("1")
def _ctz(x): return (x & -x).bit_length() - 1
def _op(cls, merge): return OP_D if cls == 2 else OP_X if cls == 1 else (OP_M if merge else OP_EQ)


def walk(nib, pos, span, L, merge=False):
    """one wave: -> (aln [5] or None, [(length, op)]) of the pair with span = (q_begin, q_end, t_begin, t_end) and a read of L letters"""
    qb, qe, tb, te = span
    if tb < 0 or te < tb or qb < 0 or qe < qb or qe >= L: return None, []
    out = {}
    def put(i, length, op):
        assert i not in out, "op %d written twice" % i
        out[i] = (int(length), op)
    nops = 1 if qb > 0 else 0
    if qb > 0: put(0, qb, OP_S)
    have_open, open_idx, open_len = False, 0, 0
    carry_cls = carry_flag = 0; n_x = n_d = 0
    for base in range(tb & ~63, te + 1, 64):
        valid = [tb <= base + l <= te for l in range(64)]
        nb = [int(nib[base + l]) if valid[l] else 0 for l in range(64)]
        for l in range(64):
            assert not valid[l] or nb[l] != GARBAGE_NIB, "unwritten nibble read at %d" % (base + l)
        code = [v & 7 for v in nb]; flag = [v >> 3 for v in nb]
        cls = [2 if c == REC_DEL else (0 if (merge or c == REC_EQ) else 1) for c in code]
        pc = [carry_cls] + cls[:63]; pf = [carry_flag] + flag[:63]
        insb = [valid[l] and base + l > tb and pf[l] == 1 and pc[l] != 2 and cls[l] != 2 for l in range(64)]
        start = [valid[l] and (base + l == tb or cls[l] != pc[l] or insb[l]) for l in range(64)]
        S = sum(1 << l for l in range(64) if start[l]); I = sum(1 << l for l in range(64) if insb[l]); V = sum(1 << l for l in range(64) if valid[l])
        n_x += sum(valid[l] and code[l] != REC_EQ and code[l] != REC_DEL for l in range(64)); n_d += sum(valid[l] and code[l] == REC_DEL for l in range(64))
        v0, v1 = _ctz(V), V.bit_length() - 1
        my = [nops + _popc(S & ((1 << l) - 1)) + _popc(I & ((1 << l) - 1)) for l in range(64)]
        for l in range(64):
            if insb[l]:
                a, b = int(pos[base + l - 1]), int(pos[base + l])
                assert a != GARBAGE_POS and b != GARBAGE_POS, "position read at a cell that holds none"
                put(my[l], b - a - 1, OP_I)
        if have_open: open_len += (_ctz(S) if S else v1 + 1) - v0
        if S:
            if have_open: put(open_idx, open_len, _op(carry_cls, merge))
            for l in range(64):
                if start[l]:
                    above = S & ((MASK64 << l) << 1) & MASK64
                    if above: put(my[l] + insb[l], _ctz(above) - l, _op(cls[l], merge))
            last = S.bit_length() - 1
            open_idx = nops + _popc(S & ((1 << last) - 1)) + _popc(I & ((2 << last) - 1) & MASK64)
            open_len = v1 - last + 1; have_open = True
        nops += _popc(S) + _popc(I)
        carry_cls, carry_flag = cls[v1], flag[v1]
    put(open_idx, open_len, _op(carry_cls, merge))
    if L - 1 - qe > 0: put(nops, L - 1 - qe, OP_S); nops += 1
    assert sorted(out) == list(range(nops)), "ops %s of %d" % (sorted(out), nops)
    nm = n_x + n_d + (qe - qb + 1) - ((te - tb + 1) - n_d)
    return [tb, te, qb, qe, nm], [out[i] for i in range(nops)]
