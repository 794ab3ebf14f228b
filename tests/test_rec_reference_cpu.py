"""CPU: the oracle-free column source (tests/columns_reference.py) against the project's C oracle, and the edge families of tests/rec_cases.py.

1. Per family, over the distinct oriented (read, centre) pairs of every case: columns_reference.ed_ops == ongsid_i_ed_ops, and columns_reference.strands == the strands
   of ongsid_polish_trace_aln.  The oracle-based references of the five consumers therefore stand on the independent anchor too.
2. The five references with source=columns_reference == the same references with the oracle as source, on every case (the plumbing of `source=`).
3. What each family promises, asserted on the reference's columns (regular expressions over the column string '=XID', the counted span, the tags).
4. ed_cases families a - g through the same ed_ops comparison, and a scalar rebuild of ed_ops from ed_reference.scalar_align_pair.
5. Sensitivity: ed_ops perturbed in one rule at a time must DIFFER from the oracle on the families built to see that rule.  What was found:
     up_left_swapped  (centre-only preferred to read-only where both continue a cheapest path and no diagonal does): differs on case "ties", listed reads 289, 291, 293,
                      tag ("up_or_left", ...) - reads built for that tie; the repeat reads do not see it, a gap in a repeat is placed by the diagonal preference alone;
     rightmost_end    (the rightmost minimum of the last row): differs on case "ties", listed reads 280, 283, 286, tag ("twice", ...): the read moves to the
                      second copy (elsewhere the minimum of the last row is attained once);
     trailing_I_in    (the 'I' run behind the last diagonal column put in front of it, as if it were counted): differs on case "ends", listed read 2, tag trail_I, and on 9 more (lead_trail_I,
                      I_behind_last, all_N_but_seed).
"""
import re
import numpy as np
import pytest
import ed_cases
import ed_reference as ed
import columns_reference as cr
import rec_cases
import rec_expected as rx
import support_reference as sr
from cigar_reference import counted

FAMILIES = sorted(rec_cases.FAMILIES)
CAP = 40e6
LETTERS = "=XID"


def _u8(s):
    return np.frombuffer(s.encode(), dtype=np.uint8)


def _string(ops):
    return "".join(LETTERS[v] for v in ops)


def distinct_pairs(case):
    """{(oriented read, centre): first listed read} over the reads with a strand"""
    out = {}
    for x, (s, r, _) in enumerate(rx.listed_columns(case)):
        if s >= 0: out.setdefault((r, case.centres[rx.group_of(case, x)]), x)
    return out


def ops_differences(oracle, case, ops_fn=cr.ed_ops):
    """listed reads (the first of each distinct pair) whose column list from ops_fn differs from the oracle's"""
    return [x for (r, c), x in distinct_pairs(case).items() if not np.array_equal(sr.ed_ops(oracle, _u8(r), _u8(c)), ops_fn(r, c))]


@pytest.mark.parametrize("family", FAMILIES)
def test_columns_and_strands_equal_the_oracle(oracle, family):
    pairs = set()                                                          # distinct over the family: the calls of clip and of class share their pairs
    for case in rec_cases.cases(family):
        _, rs = rx.read_sets(case)
        mine = cr.strands(case.centres, rs, case.grp_off, case.read_order, case.k, case.w)
        theirs = sr.strands(oracle, case.centres, rs, case.grp_off, case.read_order, case.k, case.w)
        bad = np.nonzero(mine != theirs)[0]
        assert len(bad) == 0, "%s: strand of listed read %d (%s): reference %d, oracle %d" % (case.name, bad[0], case.tags[bad[0]], mine[bad[0]], theirs[bad[0]])
        bad = ops_differences(oracle, case)
        assert not bad, "%s: columns of listed read %d (%s) differ from the oracle's" % (case.name, bad[0], case.tags[bad[0]])
        pairs |= set(distinct_pairs(case))
    cells = sum(len(r) * len(c) for r, c in pairs)
    print("%s: %d calls, %d listed reads, %d distinct pairs, %.1f M cells" % (family, len(rec_cases.cases(family)), sum(int(c.grp_off[-1]) for c in rec_cases.cases(family)), len(pairs), cells / 1e6))
    assert cells <= CAP, (family, cells)


@pytest.mark.parametrize("family", FAMILIES)
def test_references_agree_between_sources(oracle, family):
    """source=columns_reference against the oracle as source: through the default (source=None: ongsid_i_ed_ops once per LISTED read) in the families of few listed
    reads, through the same two oracle functions behind a cache per distinct pair in all of them"""
    cached = _CachedOracle(oracle)
    for case in rec_cases.cases(family):
        for what in rx.CALLS:
            a = rx.expected(case, what); b = rx.expected(case, what, oracle=oracle, source=cached)
            assert len(a) == len(b)
            for k, (u, v) in enumerate(zip(a, b)):
                assert (u is None and v is None) or (u.dtype == v.dtype and np.array_equal(u, v)), (case.name, what, k)
            if family not in ("pack", "ends", "ties", "clip"): continue
            b = rx.expected(case, what, oracle=oracle, source=None)
            assert len(a) == len(b)
            for k, (u, v) in enumerate(zip(a, b)):
                assert (u is None and v is None) or (u.dtype == v.dtype and np.array_equal(u, v)), (case.name, what, k)


class _CachedOracle:
    """the oracle as a column source: ongsid_i_ed_ops once per distinct (oriented read, centre), the strand call once per distinct (read, centre, k, w)"""
    __name__ = "cached_oracle"

    def __init__(self, oracle):
        self.oracle, self.ops, self.st = oracle, {}, {}

    def ed_ops(self, read, centre):
        key = (bytes(read), bytes(centre))
        if key not in self.ops: self.ops[key] = sr.ed_ops(self.oracle, read, centre)
        return self.ops[key]

    def strands(self, centres, rs, grp_off, read_order, k, w):
        grp_off = np.asarray(grp_off, dtype=np.uint64); ro = np.asarray(read_order)
        key = lambda g, x: (bytes(rs.seq[int(rs.off[int(ro[x])]):int(rs.off[int(ro[x]) + 1])]), centres[g], k, w)
        first, off = [], [0]                                                # one listed read per key the cache does not hold yet, group by group
        for g in range(len(centres)):
            new = {}
            for x in range(int(grp_off[g]), int(grp_off[g + 1])):
                if key(g, x) not in self.st: new.setdefault(key(g, x), x)
            first += list(new.items()); off.append(len(first))
        if first:
            st = sr.strands(self.oracle, centres, rs, np.array(off, dtype=np.uint64), np.array([int(ro[x]) for _, x in first], dtype=np.uint32), k, w)
            for (kk, _), s in zip(first, st.tolist()): self.st[kk] = s
        return np.array([self.st[key(g, x)] for g in range(len(centres)) for x in range(int(grp_off[g]), int(grp_off[g + 1]))], dtype=np.int8)


def _info(case):
    """per listed read with a strand: (x, tag, column string, first and last counted column or None, oriented read, centre)"""
    out = []
    for x, (s, r, ops) in enumerate(rx.listed_columns(case)):
        if s < 0: continue
        out.append((x, case.tags[x], _string(ops), counted(np.asarray(ops), case.clip), r, case.centres[rx.group_of(case, x)]))
    return out


def _positions(s):
    """read and centre position of every column of a column string"""
    q, t, qi, ti = [], [], 0, 0
    for ch in s:
        q.append(qi); t.append(ti)
        if ch != "D": qi += 1
        if ch != "I": ti += 1
    return q, t


@pytest.mark.parametrize("family", FAMILIES)
def test_every_read_has_a_strand_and_a_column_unless_tagged(family):
    for case in rec_cases.cases(family):
        cols = rx.listed_columns(case)
        for x, (s, r, ops) in enumerate(cols):
            tag = case.tags[x][0]
            if tag == "no_strand": assert s < 0, (case.name, x, case.tags[x]); continue
            assert s >= 0, (case.name, x, case.tags[x], "no strand")
            assert (counted(np.asarray(ops), case.clip) is None) == (tag == "no_column"), (case.name, x, case.tags[x])
            if len(case.tags[x]) and case.tags[x][-1] in (0, 1) and tag not in ("slice", "equal", "twice") and family != "pack":
                assert s == case.tags[x][-1], (case.name, x, case.tags[x], s)       # the strand the builder meant


def test_family_pack():
    (case,) = rec_cases.cases("pack")
    lens = [len(c) for c in case.centres]; sizes = np.diff(case.grp_off.astype(np.int64)).tolist()
    assert set(rec_cases.PACK_LENS) <= set(lens) and 0 in lens and 0 in sizes and {1, 63, 65} <= set(sizes)
    assert sizes[lens.index(0)] > 0                                         # the empty centre has listed reads
    st = [s for s, _, _ in rx.listed_columns(case)]
    # reads without a strand sit between reads with one: the pair order shifts against the listed order, by different amounts
    shift = sorted({x - sum(1 for s in st[:x] if s >= 0) for x in range(len(st)) if st[x] >= 0})
    assert len(shift) >= 10, shift
    info = _info(case)
    tb, te = set(), set()
    for x, tag, s, c, r, C in info:
        q, t = _positions(s)
        tb.add((t[c[0]] % 64, len(C))); te.add((t[c[1]] % 64, len(C)))
    for m in (128, 129, 257, 520):                                          # first and last counted position: on the flush boundaries (4, 8 and 64 positions) and one off
        b = {p for p, l in tb if l == m}; e = {p for p, l in te if l == m}
        assert {0, 1, 3, 4, 5, 7} <= {p % 8 for p in b} and {0, 3, 6, 7} <= {p % 8 for p in e} and {0, 1, 63} <= b and {62, 63, 0} <= e, (m, sorted(b), sorted(e))
    assert any("I" in s[c[0]:c[1] + 1] and "D" in s[c[0]:c[1] + 1] for _, tag, s, c, _, _ in info if tag[0] == "mutated")
    assert sum(1 for s in st if s == 1) >= 20 and (1 << 16) > max(map(len, case.reads))


def test_family_ends():
    (case,) = rec_cases.cases("ends")
    info = _info(case)
    def some(tagname, rx_):
        hits = [x for x, tag, s, c, _, _ in info if tag[0] == tagname and re.search(rx_, s)]
        assert hits, (tagname, rx_)
    some("lead_I", r"^I+[=X]"); some("trail_I", r"[=X]I+$"); some("lead_trail_I", r"^I+[=X].*[=X]I+$")
    some("I_front_first", r"^I+[=X]")                                   # an 'I' run directly in front of the first counted column ...
    some("I_behind_last", r"=I+D+$")                                    # ... directly behind the last one, inside the centre ...
    some("I_behind_second_last", r"=I+=D+$")                            # ... and behind the second-to-last (the last INS bit that counts)
    some("D_then_eq", r"=D+=")
    seen = set()
    for x, tag, s, c, r, C in info:
        q, t = _positions(s)
        for col in range(c[0], c[1] + 1):
            if s[col] == "X": seen.add((r[q[col]] if r[q[col]] == "N" else "acgt" if tag[0] != "N_in_centre" else r[q[col]], C[t[col]] == "N"))
            if s[col] == "=": assert r[q[col]] == C[t[col]] != "N"
    assert {("N", False), ("N", True), ("A", True), ("C", True), ("G", True), ("T", True)} <= seen, seen
    assert any(tag[0] == "all_N_but_seed" and s.count("=") >= 55 and s.count("X") >= 3 for _, tag, s, _, _, _ in info)
    assert any(tag[0] == "N_in_centre_deleted" and re.search(r"=D=", s) for _, tag, s, _, _, _ in info)
    assert sorted(len(c) for c in case.centres) == [130, 300]


def test_family_ties():
    (case,) = rec_cases.cases("ties")
    info = _info(case)
    seen = set()
    for x, tag, s, c, r, C in info:
        if tag[0] == "repeat":
            _, unit, n, d, strand = tag
            body = s[c[0]:c[1] + 1]
            assert "X" not in body and body.count("D") == max(-d, 0) and body.count("I") == max(d, 0), (x, tag, s)     # the cheapest path costs |d|: where the gap sits is a tie
            if d:
                q, t = _positions(s); g = rx.group_of(case, x)
                a = (len(C) - len(unit) * n) // 2; b = a + len(unit) * n                                                 # the repeat as built, widened by what the random flanks add to it
                while a > 0 and C[a - 1] == C[a - 1 + len(unit)]: a -= 1
                while b < len(C) and C[b] == C[b - len(unit)]: b += 1
                gaps = [t[col] for col in range(len(s)) if s[col] in "ID"]
                assert all(a <= p <= b for p in gaps), (x, tag, gaps, a, b)
                if len(unit) == 1: assert gaps[0] == a, (x, tag, gaps, a)                                               # diagonal first, walking backwards: the gap ends up at the run's first position
            seen.add((len(unit), n, d))
        if tag[0] == "twice":
            q, t = _positions(s)
            assert t[c[0]] == 17 and set(s[c[0]:c[1] + 1]) == {"="}, (x, tag)                                            # the leftmost end column: the first copy
        if tag[0] == "up_or_left": seen.add("up_or_left")
    assert {(1, n, d) for n in range(2, 21) for d in (-2, -1, 1, 2)} <= seen
    assert {(2, n, d) for n in (2, 3, 5, 8, 10) for d in (-2, -1, 1, 2)} | {(3, n, d) for n in (2, 3, 5, 7) for d in (-2, -1, 1, 2)} <= seen
    assert {63, 64, 65, 127, 128, 129} <= {len(c) for c in case.centres}


def test_family_clip():
    on, off = rec_cases.cases("clip")
    assert on.clip and not off.clip and on.reads == off.reads and on.centres == off.centres
    a, b = _info(on), _info(off)
    runs = lambda s: [len(r) for r in re.findall(r"=+", s)]
    n_diff = 0
    for (x, tag, s, c, r, C), (_, _, s0, c0, _, _) in zip(a, b):
        assert s == s0
        name = tag[1] if tag[0] == "no_column" else tag[0]
        if name == "head_run": assert re.match(r"^D*={%d}X" % tag[1], s) and (c[0] == s.index("=")) == (tag[1] >= 15), (x, tag, s)
        if name == "tail_run": assert re.search(r"X={%d}D*$" % tag[1], s) and (c[1] == s.rindex("=")) == (tag[1] >= 15), (x, tag, s)
        if name == "single_run": assert sorted(runs(s))[-2:][0] < 15 and max(runs(s)) == 15 and c[1] - c[0] == 14 and re.search(r"X={15}X", s), (x, tag, s)
        if name == "single_run_gap": assert sum(l >= 15 for l in runs(s)) == 1 and c[1] - c[0] == 14 and re.search(r"I={15}D", s), (x, tag, s)
        if name == "start_run": assert re.match(r"^D*={20}X", s) and c[0] == s.index("=") and c[1] == c[0] + 19, (x, tag, s)
        if name == "no_run": assert max(runs(s)) < 15 and c is None and c0 is not None, (x, tag, s)
        if name == "ended_by_gap": assert re.search(r"X={15}D", s) and re.search(r"={16}I", s) and re.search(r"X={15}I", s) and s[c[0] - 1] == "X" and s[c[1] + 1] == "I", (x, tag, s)
        if name == "ended_by_X": assert re.search(r"I={15}X", s) and re.search(r"D={15}X", s) and s[c[0] - 1] == "I" and s[c[1] + 1] == "X", (x, tag, s)
        if name == "edits_outside":
            head, tail = s[c0[0]:c[0]], s[c[1] + 1:c0[1] + 1]
            assert all(ch in head for ch in "XID") and all(ch in tail for ch in "XID"), (x, tag, s)
        if name == "ins_before_first_run": assert s[c[0] - 1] == "I" and s[c[0] - 2] == "=", (x, tag, s)       # the INS bit sits on the column in front of the first counted one
        if c is not None and c != c0: n_diff += 1
    assert n_diff >= 40
    for what in ("support", "cigar", "errprof"):
        assert not all(np.array_equal(u, v) for u, v in zip(rx.expected(on, what), rx.expected(off, what)) if u is not None), what


def test_family_inst():
    cs = rec_cases.cases("inst")
    assert [max(map(len, c.reads)) for c in cs] == rec_cases.INST_LENS
    for case in cs:
        info = _info(case)
        assert len(info) == 96 and any(tag[0] == "short_slice" for _, tag, *_ in info)
        assert len({r for *_, r, _ in info}) == 4
        for x, tag, s, c, r, C in info:
            if tag[0] == "long": assert 0.002 < 1 - s.count("=") / len(r) < 0.06, (case.name, x, tag)
        assert any("I" in s[c[0]:c[1] + 1] for _, _, s, c, _, _ in info) and any("D" in s[c[0]:c[1] + 1] for _, _, s, c, _, _ in info), case.name


def _distance(s):
    body = s.strip("D")
    return len(body) - body.count("=")


def test_family_band():
    for case, K in zip(rec_cases.cases("band"), rec_cases.BAND_KS):
        info = _info(case)
        assert len(info) == 1024 and len(case.centres) == 30 and np.diff(case.grp_off.astype(np.int64)).tolist()[14:] == [50] + [64] * 15
        d = {}
        for x, tag, s, c, r, C in info: d.setdefault(tag[:-1], _distance(s))
        dist = sorted(d.values())
        assert {K - 1, K, K + 1} <= set(dist) and dist[-1] >= 1.5 * K and sum(v > K for v in dist) >= 5 and sum(v <= K for v in dist) >= 5, (K, d)
        assert {t[0] for t in d} == {"spread", "qblock", "tblock"}
        lens = {len(r) - len(C) for *_, r, C in info}
        assert min(lens) < -K // 2 and max(lens) > K // 2                      # reads longer and shorter than their centres: the mixed bundle's band is wide


def test_family_class():
    cs = rec_cases.cases("class")
    assert [int(c.grp_off[-1]) for c in cs] == [4096, 4097, 4096, 4097, 4096]
    bounds = [256, 512, 768, 896]
    for case, drop in zip(cs, (None, None, 2, 3, 4)):
        info = _info(case)
        assert len(info) == int(case.grp_off[-1])                            # every read has a strand: 4 096 PAIRS or more
        cls = np.searchsorted(bounds, [len(r) for *_, r, _ in info], side="left")
        have = set(cls.tolist())
        assert have == set(range(5)) - ({drop} if drop is not None else set()), (case.name, have)
        d = {}
        for x, tag, s, c, r, C in info: d.setdefault((r, C), _distance(s))
        dist = sorted(d.values())
        assert dist[0] < 20 and sum(96 < v <= 180 for v in dist) >= 1 and dist[-1] > 180, (case.name, dist)
        assert max(len(c) for c in case.centres) <= 1100
        # bundles of 64 pairs in pair order that hold reads of more than one class (what the launches without classes run; the class launches bundle each class's own list):
        # at least every second group boundary falls inside a bundle
        mixed = [lo for lo in range(0, len(cls), 64) if len(set(cls[lo:lo + 64].tolist())) > 1]
        assert len(mixed) >= (len(case.centres) - 1) // 2, (case.name, len(mixed))


@pytest.mark.parametrize("family", sorted(ed_cases.FAMILIES))
def test_ed_cases_columns_equal_the_oracle(oracle, family):
    pairs = {}
    for case in ed_cases.cases(family):
        for qi, ti in zip(case.q_idx.tolist(), case.t_idx.tolist()): pairs[(case.queries[qi], case.targets[ti])] = case.name
    assert sum(len(q) * len(t) for q, t in pairs) <= 60e6
    for (q, t), name in pairs.items():
        mine = cr.ops_of_path(q, t, ed.align_pair(q, t)[2]) if (len(q) and len(ed.align_pair(q, t)[2])) else cr.ed_ops(q, t)      # (not cached: these pairs are used once)
        assert np.array_equal(sr.ed_ops(oracle, _u8(q), _u8(t)), mine), (name, len(q), len(t))
        cr._ops.pop((q, t), None)


def test_ed_ops_from_the_scalar_reference():
    rng = np.random.default_rng(5)
    for it in range(50):
        n, m = int(rng.integers(0, 24)), int(rng.integers(0, 30))
        alphabet = "ACGT" if it % 3 else "ACGTNacgt"
        t = "".join(alphabet[x] for x in rng.integers(0, len(alphabet), m))
        q = ed_cases.mutate(rng, t[int(rng.integers(0, 4)):], 0.1, 0.1, 0.1)[:n] if (it % 2 and it % 3) else "".join(alphabet[x] for x in rng.integers(0, len(alphabet), n))
        d, end, cols = ed.scalar_align_pair(q, t)
        if len(q) == 0: exp = [3] * len(t)
        elif not cols: exp = [3] * end + [2] * len(q) + [3] * (len(t) - end)
        else:
            exp = []; pq, pt = -1, -1
            for qi, ti in cols:
                exp += [3] * (ti - pt - 1) + [2] * (qi - pq - 1)
                exp.append(0 if (q[qi] in "ACGTacgt" and q[qi].upper() == t[ti].upper()) else 1); pq, pt = qi, ti
            exp += [2] * (len(q) - 1 - pq) + [3] * (len(t) - 1 - pt)
        got = cr.ed_ops(q, t)
        assert got.dtype == np.uint8 and got.tolist() == exp, (q, t)
        body = _string(got).strip("D")
        assert len(body) - body.count("=") == d


# ---- sensitivity: one rule changed at a time
def _traceback(q, t, swap=False, rightmost=False):
    D = ed.dp_matrix(q, t); qc, tc = ed._codes(q), ed._codes(t); n = len(qc)
    end = int(len(D[n]) - 1 - np.argmin(D[n][::-1])) if rightmost else int(np.argmin(D[n]))
    i, j, cols = n, end, []
    while i > 0:
        if j > 0:
            neq = 0 if (qc[i - 1] < 4 and qc[i - 1] == tc[j - 1]) else 1
            if D[i - 1, j - 1] + neq == D[i, j]:
                cols.append((i - 1, j - 1)); i -= 1; j -= 1
                continue
        up = D[i - 1, j] + 1 == D[i, j]; left = j > 0 and D[i, j - 1] + 1 == D[i, j]
        if (left and (swap or not up)): j -= 1
        else: i -= 1
    return end, cols[::-1]


def _perturbed(kind):
    def ops(read, centre):
        if len(read) == 0: return cr.ed_ops(read, centre)
        end, cols = _traceback(read, centre, swap=kind == "up_left_swapped", rightmost=kind == "rightmost_end")
        if not cols: return np.array([3] * end + [2] * len(read) + [3] * (len(centre) - end), dtype=np.uint8)
        out = cr.ops_of_path(read, centre, cols).tolist()
        if kind == "trailing_I_in":
            s = _string(out); m = re.search(r"([=X])(I+)(D*)$", s)
            if m: out = out[:m.start(1)] + [2] * len(m.group(2)) + [out[m.start(1)]] + [3] * len(m.group(3))
        return np.array(out, dtype=np.uint8)
    return ops


@pytest.mark.parametrize("kind,family", [("up_left_swapped", "ties"), ("rightmost_end", "ties"), ("trailing_I_in", "ends")])
def test_a_perturbed_rule_differs_from_the_oracle(oracle, kind, family):
    (case,) = rec_cases.cases(family)
    bad = ops_differences(oracle, case, _perturbed(kind))
    print(kind, case.name, [(x, case.tags[x]) for x in bad][:8], len(bad))
    assert bad, "%s: no case of %s tells the rule from its perturbation" % (kind, family)
    if kind == "rightmost_end": assert any(case.tags[x][0] == "twice" for x in bad)
    if kind == "up_left_swapped": assert any(case.tags[x][0] == "up_or_left" for x in bad)
