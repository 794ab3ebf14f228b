"""CPU: the definition of ngsid_read_cigars (tests/cigar_reference.py) keeps the invariants include/ngsid_cigar.h promises, the step logic of k_cigar_walk in Python
integers (tests/cigar_wave_model.py) equals it on rows that cross a 64-position step in every way, and the native SAM writer (fastio.write_sam, host library only)
writes what sam.parse_sam reads back."""
import os
import numpy as np
import pytest
from ngspeciesid_amd import fastio, sam
from ngspeciesid_amd._capi import ReadSet, CIGAR_OPS
from support_reference import ed_ops, _COMP
from cigar_reference import cigar_of_columns, counted, walk_record, OP_S, OP_I, OP_D, OP_EQ, OP_X, OP_M
import cigar_wave_model as wm

MATCH_OPS = (OP_M, OP_EQ, OP_X)


def _enc(s):
    return np.frombuffer(s.encode(), dtype=np.uint8)


def _random_pair(rng):
    m = int(rng.integers(1, 201)); err = float(rng.uniform(0.0, 0.4))
    centre = "".join("ACGT"[v] for v in rng.integers(4, size=m))
    a = int(rng.integers(0, max(1, m // 3))); b = m - int(rng.integers(0, max(1, m // 3)))
    body = []
    for c in centre[a:max(b, a + 1)]:
        u = rng.random()
        if u < err / 3: continue
        if u < 2 * err / 3: body.append("ACGT"[int(rng.integers(4))]); continue
        body.append(c)
        if u > 1 - err / 3: body.append("ACGT"[int(rng.integers(4))])
    over = lambda: "".join("ACGT"[v] for v in rng.integers(4, size=int(rng.integers(0, 12)))) if rng.random() < 0.5 else ""
    read = over() + "".join(body) + over()
    if not read: read = "A"
    if rng.random() < 0.3:
        i = int(rng.integers(len(read))); read = read[:i] + "N" + read[i + 1:]
    return read, centre


def _check_invariants(cols, L, clip, merge):
    a, runs = cigar_of_columns(cols, L, clip, merge)
    c = counted(cols, clip)
    if a is None:
        assert c is None and runs == []
        return None
    tb, te, qb, qe, nm = a
    assert sum(n for n, o in runs if o in (OP_M, OP_EQ, OP_X, OP_I, OP_S)) == L
    assert sum(n for n, o in runs if o in (OP_M, OP_EQ, OP_X, OP_D)) == te - tb + 1
    body = [r for r in runs if r[1] != OP_S]
    assert body[0][1] in MATCH_OPS and body[-1][1] in MATCH_OPS
    assert all(x[1] != y[1] for x, y in zip(runs[:-1], runs[1:])) and all(n > 0 for n, _ in runs)
    assert not any({x[1], y[1]} == {OP_I, OP_D} for x, y in zip(runs[:-1], runs[1:]))
    assert [o for _, o in runs].count(OP_S) == (qb > 0) + (L - 1 - qe > 0) and all(r[1] != OP_S for r in runs[1:-1])
    o = cols[c[0]:c[1] + 1]
    if not merge:                                                              # expanding the ops gives back the counted columns
        back = {OP_EQ: 0, OP_X: 1, OP_I: 2, OP_D: 3}
        assert [back[op] for n, op in body for _ in range(n)] == o.tolist()
    assert nm == int((o != 0).sum())
    assert not any({int(x), int(y)} == {2, 3} for x, y in zip(o[:-1], o[1:])), "an 'I' column touches a 'D' column inside the span"
    return a, runs


def test_reference_invariants_and_wave_model_on_random_pairs(oracle):
    rng = np.random.default_rng(2026)
    seen = 0
    for x in range(300):
        read, centre = _random_pair(rng)
        cols = ed_ops(oracle, _enc(read), _enc(centre))
        nib, pos = wm.rows_of_columns(cols, _enc(read), len(centre))
        for clip in (False, True):
            for merge in (False, True):
                ref = _check_invariants(cols, len(read), clip, merge)
                span = (-1, -1, -1, -1) if ref is None else (ref[0][2], ref[0][3], ref[0][0], ref[0][1])
                got = wm.walk(nib, pos, span, len(read), merge)
                assert got == ((None, []) if ref is None else ref), (read, centre, clip, merge)
                seen += ref is not None
    assert seen > 600


def _pair_of_body(rng, m, t0, body, lead=0, trail=0):
    """a centre of m letters, and the read and the oracle-style column list of `body` (over = X I D) placed at centre position t0 with `lead` / `trail` free read letters"""
    centre = "".join("ACGT"[v] for v in rng.integers(4, size=m))
    other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4]
    read, ti = ["T"] * lead, t0
    for c in body:
        if c == "=": read.append(centre[ti]); ti += 1
        elif c == "X": read.append(other(centre[ti])); ti += 1
        elif c == "I": read.append("G")
        else: ti += 1
    assert ti <= m
    read += ["C"] * trail
    cols = [3] * t0 + [2] * lead + ["=XID".index(c) for c in body] + [2] * trail + [3] * (m - ti)
    return np.array(cols, dtype=np.uint8), "".join(read), centre


STEP_CASES = [
    # (centre length, t_begin, body, lead, trail)
    (63, 0, "=" * 63, 0, 0), (64, 0, "=" * 64, 0, 0), (65, 0, "=" * 65, 0, 0), (128, 0, "=" * 128, 0, 0), (129, 0, "=" * 129, 0, 0),      # an '=' run over every step boundary
    (129, 0, "=" * 62 + "DDD" + "=" * 64, 0, 0),                                                       # a 'D' run over 63 | 64
    (129, 0, "=" * 63 + "D" + "=" * 65, 0, 0), (129, 0, "=" * 64 + "D" + "=" * 64, 0, 0),              # ... ending at 63, beginning at 64
    (129, 0, "=" * 63 + "XX" + "=" * 64, 2, 3), (129, 0, "=" * 64 + "X" * 64 + "=", 0, 0),             # 'X' over the boundary, a whole step of 'X'
    (130, 0, "=" * 64 + "I" + "=" * 66, 0, 0), (130, 0, "=" * 64 + "III" + "X" + "=" * 65, 0, 0),      # an insertion flagged on position 63
    (130, 0, "=" * 63 + "I" + "=" * 67, 0, 0), (130, 0, "=" * 128 + "I" + "==", 0, 0),                 # ... on 62, on 127
    (100, 0, "=" * 98 + "II" + "=", 0, 0), (65, 0, "=" * 63 + "I" + "=", 0, 4),                        # ... on t_end - 1 (with t_end = 64: across the step)
    (129, 1, "=" * 100, 0, 0), (129, 7, "=X" * 50, 3, 0), (129, 8, "=" * 121, 0, 5), (129, 63, "=" * 66, 5, 0), (129, 63, "=D" + "=" * 10, 1, 1),      # spans that begin inside a dword / a step
    (129, 64, "=I=D=X=", 0, 0), (200, 60, "X" + "=" * 3 + "D" + "=" * 70 + "I" + "X=", 9, 9),
    (80, 10, "=" * 30, 0, 6), (129, 0, "=" * 64, 0, 2), (129, 0, "=" * 128, 0, 2),                     # a flag on t_end itself (trailing read letters): no op
    (70, 5, "=", 4, 4), (70, 63, "X", 0, 3), (70, 64, "=", 2, 0), (1, 0, "=", 0, 0),                   # a one-column span
]


@pytest.mark.parametrize("case", range(len(STEP_CASES)))
def test_wave_model_equals_reference_across_steps(case):
    m, t0, body, lead, trail = STEP_CASES[case]
    rng = np.random.default_rng(100 + case)
    cols, read, centre = _pair_of_body(rng, m, t0, body, lead, trail)
    nib, pos = wm.rows_of_columns(cols, _enc(read), m)
    if trail and body[-1] in "=X":
        te = t0 + sum(c != "I" for c in body) - 1
        assert nib[te] & wm.REC_INS                                             # the flag the walk must ignore
    for merge in (False, True):
        ref = _check_invariants(cols, len(read), False, merge)
        assert ref is not None and ref[0][0] == t0
        got = wm.walk(nib, pos, (ref[0][2], ref[0][3], ref[0][0], ref[0][1]), len(read), merge)
        assert got == ref, (case, merge, got, ref)


def test_small_traceback_equals_the_oracle(oracle):
    """the rows of a pair whichever way they are made: the model's own traceback == the oracle's column list without its free centre ends"""
    rng = np.random.default_rng(7)
    for x in range(25):
        read, centre = _random_pair(rng)
        if len(centre) > 90: centre = centre[:90]
        cols, t0 = wm.traceback_columns(_enc(read), _enc(centre))
        exp = ed_ops(oracle, _enc(read), _enc(centre))
        on = np.nonzero(exp != 3)[0]; lead = int((exp[:on[0]] == 3).sum())
        assert t0 == lead and cols.tolist() == exp[on[0]:on[-1] + 1].tolist(), (read, centre)
        nib_a, pos_a = wm.rows_of_columns(cols, _enc(read), len(centre), t0); nib_b, pos_b = wm.rows_of_columns(exp, _enc(read), len(centre))
        assert np.array_equal(nib_a, nib_b) and np.array_equal(pos_a, pos_b)


# ---- the record writer
def _rc(s):
    return _COMP[_enc(s)[::-1]].tobytes().decode()


def _sam_inputs(oracle):
    rng = np.random.default_rng(31)
    targets = ["".join("ACGT"[v] for v in rng.integers(4, size=n)) for n in (150, 200)]
    reads, quals, strand, target, aln, runs_all = [], [], [], [], [], []
    for x in range(20):
        t = x % 2; c = targets[t]
        a = int(rng.integers(0, 40)); piece = list(c[a:a + 90])
        for _ in range(5): piece[int(rng.integers(len(piece)))] = "ACGT"[int(rng.integers(4))]
        del piece[20]; piece.insert(50, "A"); piece.insert(50, "C")
        fwd = "GGT" * (x % 3) + "".join(piece) + "TTG" * (x % 2)
        if x == 4: fwd = fwd[:30] + "N" + fwd[31:]
        s = 1 if x % 3 == 1 else 0
        a5, runs = cigar_of_columns(ed_ops(oracle, _enc(fwd), _enc(c)), len(fwd), False)
        assert a5 is not None
        if x == 7: s, t, a5, runs = -1, -1, [-1] * 5, []                          # the unmapped read
        reads.append(_rc(fwd) if s == 1 else fwd); quals.append("".join(chr(33 + int(v)) for v in rng.integers(2, 40, size=len(fwd))))
        strand.append(s); target.append(t); aln.append(a5); runs_all.append(runs)
    op_off = np.concatenate(([0], np.cumsum([len(r) for r in runs_all]))).astype(np.uint64)
    ops = np.array([(n << 4) | o for r in runs_all for n, o in r], dtype=np.uint32)
    names = fastio.Names.from_list(["read%d runid=abc ch=%d" % (x, x) if x % 2 else "read%d" % x for x in range(20)])
    no_qual = np.zeros(20, dtype=np.uint8); no_qual[11] = 1
    return dict(targets=targets, reads=reads, quals=quals, strand=np.array(strand, np.int8), target=np.array(target, np.int32), aln=np.array(aln, np.int32), op_off=op_off, ops=ops,
                names=names, no_qual=no_qual, rs=ReadSet.from_strings(reads, quals))


def _check_sam(path, d):
    p = sam.parse_sam(path)
    tn = ["cons_a", "cons_b"]
    assert p["header"][0] == "@HD\tVN:1.6\tSO:unknown" and p["targets"] == [("cons_a", 150), ("cons_b", 200)] and p["header"][-1].startswith("@PG")
    assert len(p["qname"]) == 20 and p["qname"].tolist() == ["read%d" % x for x in range(20)]
    cig = sam.cigar_strings(d["op_off"], d["ops"])
    for x in range(20):
        s, t = int(d["strand"][x]), int(d["target"][x])
        fwd = _rc(d["reads"][x]) if s == 1 else d["reads"][x]
        if t < 0:
            assert (p["flag"][x], p["rname"][x], p["pos"][x], p["mapq"][x], p["cigar"][x], p["nm"][x]) == (4, "*", 0, 0, "*", -1)
            assert p["seq"][x] == d["reads"][x] and p["qual"][x] == d["quals"][x]
            continue
        assert (p["flag"][x], p["rname"][x], p["pos"][x], p["mapq"][x]) == (16 if s else 0, tn[t], int(d["aln"][x][0]) + 1, 255)
        assert (p["rnext"][x], p["pnext"][x], p["tlen"][x]) == ("*", 0, 0)
        assert p["cigar"][x] == cig[x] and p["nm"][x] == int(d["aln"][x][4])
        assert p["seq"][x] == fwd                                                   # reverse-complemented on flag 16
        assert p["qual"][x] == ("*" if x == 11 else (d["quals"][x][::-1] if s else d["quals"][x]))
        ops = sam.cigar_ops(p["cigar"][x])
        assert sum(n for n, o in ops if o in sam.READ_OPS) == len(p["seq"][x])
        nm, used = walk_record(ops, p["seq"][x], d["targets"][t], int(p["pos"][x]))
        assert nm == p["nm"][x] and used == int(d["aln"][x][1]) - int(d["aln"][x][0]) + 1
    assert (p["flag"] == 16).sum() >= 5 and (p["flag"] == 0).sum() >= 10 and any("X" in c for c in p["cigar"]) and any("S" in c for c in p["cigar"])


def _write(path, d, **kw):
    head = sam.header(["cons_a", "cons_b"], [150, 200], "test")
    fastio.write_sam(path, head, np.arange(20), d["names"], d["rs"], d["strand"], d["target"], ["cons_a", "cons_b"], d["aln"], d["op_off"], d["ops"], no_qual=d["no_qual"], **kw)


def test_write_sam_round_trip(oracle, tmp_path):
    d = _sam_inputs(oracle)
    path = str(tmp_path / "a.sam")
    _write(path, d)
    _check_sam(path, d)
    # a read set without qualities: '*' everywhere
    rs = ReadSet.from_strings(d["reads"])
    fastio.write_sam(str(tmp_path / "b.sam"), sam.header(["cons_a", "cons_b"], [150, 200]), np.arange(20), d["names"], rs, d["strand"], d["target"], ["cons_a", "cons_b"], d["aln"], d["op_off"], d["ops"])
    assert set(sam.parse_sam(str(tmp_path / "b.sam"))["qual"].tolist()) == {"*"}
    # per-read name suffixes: appended to a name without a blank only (the name is cut at its first blank)
    sfx = fastio._csr(["_s%d" % x for x in range(20)])
    _write(str(tmp_path / "c.sam"), d, suffixes=sfx)
    assert sam.parse_sam(str(tmp_path / "c.sam"))["qname"].tolist() == ["read%d" % x if x % 2 else "read%d_s%d" % (x, x) for x in range(20)]


def test_write_sam_background_job_and_unwritable_path(oracle, tmp_path):
    d = _sam_inputs(oracle)
    jobs = fastio.NativeJobs()
    path = str(tmp_path / "bg.sam")
    _write(path, d, jobs=jobs)
    jobs.wait()
    _check_sam(path, d)
    with pytest.raises(OSError):
        _write(str(tmp_path / "no_such_folder" / "x.sam"), d)
    jobs = fastio.NativeJobs()
    _write(str(tmp_path / "no_such_folder" / "y.sam"), d, jobs=jobs)
    with pytest.raises(OSError):
        jobs.wait()


def test_cigar_strings():
    assert sam.cigar_strings([0, 3, 3, 5], [(3 << 4) | 4, (10 << 4) | 7, (1 << 4) | 8, (2 << 4) | 0, (300 << 4) | 2]) == ["3S10=1X", "*", "2M300D"]
    assert sam.cigar_ops("3S10=1X") == [(3, "S"), (10, "="), (1, "X")] and sam.cigar_ops("*") == [] and CIGAR_OPS[7] == "=" and CIGAR_OPS[8] == "X"
