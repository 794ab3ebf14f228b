"""CPU: the numpy restatement of ngsid_recruit (tests/recruit_reference.py) against the host locator, the Python-int model of the blocked column
(tests/recruit_block_model.py) against the restatement, the policy of ngspeciesid_amd/recruit.py on hand-made hit arrays, and its two tables."""
import ctypes as C
import os, re
import numpy as np
import pytest
import recruit_block_model as model
import recruit_cases as cases
import recruit_reference as ref
from ngspeciesid_amd import recruit
from ngspeciesid_amd._capi import ReadSet, RECRUIT_FIELDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (a) the reference against the host locator
@pytest.mark.parametrize("name", cases.NAMES)
def test_reference_is_the_host_locator(oracle, name):
    """every (pattern strand, read) pair of the case: ed and end of the reference are those of ongsid_host_infix_locate(p, m, x, L, k_c, iupac = 0)"""
    fn = oracle.lib.ongsid_host_infix_locate
    ed, st, en = C.c_int32(), C.c_int32(), C.c_int32()
    n = n_hit = 0
    for p, x, k in cases.pair_strands(name):
        assert fn(p.encode(), C.c_int32(len(p)), x.encode(), C.c_int32(len(x)), C.c_int32(k), C.c_int32(0), C.byref(ed), C.byref(st), C.byref(en)) == 0
        got = ref.locate(p, x, k)
        assert (got if got else (-1, -1)) == (ed.value, en.value), (name, len(p), len(x), k)
        n += 1; n_hit += got is not None
    assert n > 0 and 0 < n_hit < n                                      # hits and misses both occur in every case


def test_cutoff_cases_hold_real_hits():
    """the condition on the cut-off cases: the reference alone finds a hit on at least 90 % of the planted reads (else the comparison would be of -1 against -1)"""
    exp = cases.expected("cutoff")
    planted = cases.CUTOFF_PLANTED
    assert len(planted) == 49 and (exp[planted, 0] >= 0).mean() >= 0.9
    others = np.setdiff1d(np.arange(len(exp)), planted)
    assert (exp[others, 0] < 0).all()                                   # 63 lanes of the last wave match nothing


def test_reference_on_hand_made_pairs():
    assert ref.last_row("AC", "GACA").tolist() == [2, 1, 0, 1]          # AC against G; A; AC; (A)CA with the last letter inserted
    assert ref.locate("ACGT", "TTACGTTT", 0) == (0, 5) and ref.locate("ACGT", "", 3) is None
    assert ref.locate("AAAA", "AAAAAA", 9) == (0, 3)                    # the smallest end
    assert ref.locate("ACGT", "ACTT", 0) is None and ref.locate("ACGT", "ACTT", 1) == (1, 2)      # ACT with G deleted ends at 2; ACTT with a substitution at 3
    assert ref.locate("N", "ANA", 0) == (0, 1) and ref.locate("A", "NNN", 0) is None              # N equals only N
    assert ref.revcomp("ACGTN") == "NACGT"
    assert ref.pair("AACC", "GGTT", 0) == (0, 1, 3) and ref.pair("AACC", "GGTT", 0, both_strands=False) is None
    assert ref.pair("ACGT", "ACGT", 0) == (0, 0, 3)                     # its own reverse complement: strand 0
    h = ref.recruit(["AACCGG", "TTTTTT", ""], [0, 3], ["AACC", "AACG", "AACC"], [0, 3], [1, 1, 1])
    assert h.tolist() == [[0, 0, 0, 3, 2, 0], list(ref.NONE), list(ref.NONE)]


@pytest.mark.parametrize("name", ("read_lengths", "bounds", "reduction_both"))
def test_rows_of_many_reads_at_once(name):
    """the reference computes a table row for all reads of a group at once; read by read it gives the same"""
    c = cases.build(name)
    for g in range(len(c["read_off"]) - 1):
        reads = c["reads"][int(c["read_off"][g]):int(c["read_off"][g + 1])]
        for ci in range(int(c["cons_off"][g]), int(c["cons_off"][g + 1])):
            for p in (c["cons"][ci], ref.revcomp(c["cons"][ci])):
                assert ref.locate_many(p, reads, c["max_ed"][ci]) == [ref.locate(p, x, c["max_ed"][ci]) for x in reads]
    exp = cases.expected(name)
    for g in range(len(c["read_off"]) - 1):
        for r in range(int(c["read_off"][g]), int(c["read_off"][g + 1])):
            found = sorted((h[0], ci, h[1], h[2]) for ci in range(int(c["cons_off"][g]), int(c["cons_off"][g + 1]))
                           for h in [ref.pair(c["cons"][ci], c["reads"][r], c["max_ed"][ci], c["both"])] if h is not None)
            want = list(ref.NONE)
            if found: want[:4] = [found[0][1], found[0][0], found[0][2], found[0][3]]
            if len(found) > 1: want[4:] = [found[1][1], found[1][0]]
            assert exp[r].tolist() == want


# ---- (b) the blocked column
def _model_pairs():
    out = []
    for p, x, k in cases.pair_strands("pattern_lengths"):
        if len(p) <= 513: out.append((p, x, k))
    out += list(cases.pair_strands("carry_chains"))
    big = [t for t in cases.pair_strands("pattern_lengths") if len(t[0]) == 2048]
    return out + big[:2]


def test_block_model_is_the_table():
    """W words with hin / hout between the blocks and the score at row m - 1 give the last row of the table, word boundaries and carry chains included"""
    n = 0
    for p, x, k in _model_pairs():
        assert model.last_row(p, x) == ref.last_row(p, x).tolist(), (len(p), len(x))
        assert model.locate(p, x, k) == ref.locate(p, x, k)
        n += 1
    assert n > 200


def test_block_model_with_the_cut_off_rule():
    """the lanes of a wave under the wave-uniform last-active-block rule report what the plain column reports, and the rule skips block steps"""
    c = cases.build("cutoff")
    done = plain = 0
    for g in range(len(c["read_off"]) - 1):
        reads = c["reads"][int(c["read_off"][g]):int(c["read_off"][g + 1])]
        if g < 2: reads = reads[:8]
        for ci in range(int(c["cons_off"][g]), int(c["cons_off"][g + 1])):
            for p in (c["cons"][ci], ref.revcomp(c["cons"][ci])):
                k = min(int(c["max_ed"][ci]), len(p) - 1)
                got, d, t = model.locate_cutoff(p, reads, k)
                assert got == [ref.locate(p, x, k) for x in reads]
                done += d; plain += t
    assert 0 < done < plain
    # word boundaries and carry chains, one read per wave and all reads of the group in one wave
    for name in ("carry_chains", "read_lengths", "bounds"):
        c = cases.build(name)
        for g in range(len(c["read_off"]) - 1):
            reads = c["reads"][int(c["read_off"][g]):int(c["read_off"][g + 1])]
            for ci in range(int(c["cons_off"][g]), int(c["cons_off"][g + 1])):
                p = c["cons"][ci]; k = min(int(c["max_ed"][ci]), len(p) - 1)
                want = [ref.locate(p, x, k) for x in reads]
                assert model.locate_cutoff(p, reads, k)[0] == want
                assert [model.locate_cutoff(p, [x], k)[0][0] for x in reads[:6]] == want[:6]
    for p, x, k in _model_pairs()[::7]:
        assert model.locate_cutoff(p, [x], k)[0] == [ref.locate(p, x, k)]


# ---- (c) the policy
def test_thresholds():
    assert recruit.default_min_identity(7.0) == pytest.approx(0.80047, abs=1e-5)
    assert recruit.thresholds([650, 5, 1, 2048], 0.8).tolist() == [130, 1, 0, 409]
    assert recruit.thresholds([100], 1.0).tolist() == [0] and recruit.thresholds([100], 0.0).tolist() == [100]
    assert recruit.thresholds([650]).tolist() == [129] and recruit.thresholds([650], q=10.0).tolist() == [65]      # 0.19953 x 650 = 129.7; 0.1 x 650
    assert recruit.thresholds([]).dtype == np.int32 and len(recruit.thresholds([])) == 0
    with pytest.raises(ValueError):
        recruit.thresholds([10], 1.5)


HITS = np.array([[0, 3, 0, 99, 1, 3],        # an exact tie: ambiguous at every margin
                 [1, 2, 1, 80, 0, 3],        # one edit apart: assigned at margin 1, ambiguous at 2
                 [0, 5, 0, 70, 1, 9],        # four apart
                 [1, 0, 0, 60, -1, -1],      # no second consensus
                 [-1, -1, 0, -1, -1, -1],    # nothing
                 [0, 7, 1, 50, -1, -1]], dtype=np.int32)


def test_assign_margins_and_ties():
    U, A, M = recruit.UNASSIGNED, recruit.ASSIGNED, recruit.AMBIGUOUS
    assert recruit.assign(HITS).tolist() == [M, A, A, A, U, A]
    assert recruit.assign(HITS, min_margin=2).tolist() == [M, M, A, A, U, A]
    assert recruit.assign(HITS, min_margin=5).tolist() == [M, M, M, A, U, A]
    assert recruit.assign(HITS, min_margin=0).tolist() == [A, A, A, A, U, A]
    assert recruit.assign(np.zeros((0, 6), np.int32)).tolist() == [] and recruit.assign(HITS).dtype == np.int8
    assert recruit.STATUS_NAMES[U] == "unassigned" and recruit.STATUS_NAMES[A] == "assigned" and recruit.STATUS_NAMES[M] == "ambiguous"
    assert RECRUIT_FIELDS == ("cons", "ed", "strand", "end", "cons2", "ed2")


def test_recount_splits():
    origin = [0, 0, 1, -1, -1, 1]              # reads 0, 1 in clusters of centre 0; 2, 5 of centre 1; 3, 4 in none
    got = recruit.recount(HITS, recruit.assign(HITS), 2, origin)
    assert got == dict(centres=[dict(reads_clustered=2, reads_recruited=2, from_own_clusters=0, from_other_centres=2, from_unclustered=0),
                                dict(reads_clustered=2, reads_recruited=2, from_own_clusters=0, from_other_centres=1, from_unclustered=1)], ambiguous=1, unassigned=1)
    got = recruit.recount(HITS, recruit.assign(HITS, 0), 2, [0, 1, 0, -1, 0, 0], clustered=[40, 7])
    assert [c["reads_clustered"] for c in got["centres"]] == [40, 7]
    assert got["centres"][0] == dict(reads_clustered=40, reads_recruited=3, from_own_clusters=3, from_other_centres=0, from_unclustered=0)
    assert got["centres"][1] == dict(reads_clustered=7, reads_recruited=2, from_own_clusters=1, from_other_centres=0, from_unclustered=1)
    assert got["ambiguous"] == 0 and got["unassigned"] == 1
    for c in got["centres"]:
        assert c["reads_recruited"] == c["from_own_clusters"] + c["from_other_centres"] + c["from_unclustered"]
    # a sample with no centre: every read unassigned
    none = np.tile(np.array(ref.NONE, dtype=np.int32), (3, 1))
    assert recruit.recount(none, recruit.assign(none), 0, [-1, -1, -1]) == dict(centres=[], ambiguous=0, unassigned=3)
    assert recruit.recount(np.zeros((0, 6), np.int32), np.zeros(0, np.int8), 0, []) == dict(centres=[], ambiguous=0, unassigned=0)
    with pytest.raises(ValueError):
        recruit.recount(HITS, recruit.assign(HITS), 2, [0, 1])
    assert recruit.origin_of(6, [[4, 1], [1, 2], []]).tolist() == [-1, 0, 1, -1, 0, -1]               # a read listed twice stays with the first centre


def test_run_on_the_reference(monkeypatch):
    """run() with Api.recruit stubbed by the reference: one call for two samples and one without a centre, local centre numbers, thresholds from min_identity"""
    calls = []

    class Stub:
        def recruit(self, rs, read_off, cons, cons_off, max_ed, both_strands=True):
            reads = [rs.get(i)[0] for i in range(rs.n)]; cs = [cons.get(i)[0] for i in range(cons.n)]
            calls.append((list(read_off), list(cons_off), list(max_ed), both_strands))
            return ref.recruit(reads, read_off, cs, cons_off, max_ed, both_strands)
    rng = np.random.default_rng(5)
    a, b, c = (cases.rand(rng, m) for m in (60, 50, 40))
    reads = [a, cases.substitute(a, [3, 9]), ref.revcomp(b), "ACGT", c, cases.substitute(c, [1]), b]
    res = recruit.run(Stub(), ReadSet.from_strings(reads), [0, 4, 4, 7], [[a, b], [], [c]], min_identity=0.9, origins=[[0, -1, 0, 1], [], None], clustered=[[9, 8], [], None])
    assert calls == [([0, 4, 4, 7], [0, 2, 2, 3], [6, 5, 4], True)]
    assert res[0]["hits"][:, 0].tolist() == [0, 0, 1, -1] and res[0]["hits"][:, 2].tolist() == [0, 0, 1, 0] and res[0]["hits"][1, 1] == 2
    assert res[1]["hits"].shape == (0, 6) and res[1]["counts"] == dict(centres=[], ambiguous=0, unassigned=0)
    assert res[2]["hits"][:, 0].tolist() == [0, 0, -1] and res[2]["status"].tolist() == [1, 1, 0]                  # centre numbers local to the sample
    assert res[0]["counts"]["centres"] == [dict(reads_clustered=9, reads_recruited=2, from_own_clusters=1, from_other_centres=0, from_unclustered=1),
                                           dict(reads_clustered=8, reads_recruited=1, from_own_clusters=0, from_other_centres=1, from_unclustered=0)]
    assert res[2]["counts"]["centres"] == [dict(reads_clustered=0, reads_recruited=2, from_own_clusters=0, from_other_centres=0, from_unclustered=2)]
    with pytest.raises(ValueError):
        recruit.run(Stub(), ReadSet.from_strings(["A"]), [0, 1], [["A" * 2049]])


# ---- (d) the tables
def test_writers(tmp_path):
    st = recruit.assign(HITS)
    counts = recruit.recount(HITS, st, 2, [0, 0, 1, -1, -1, 1], clustered=[12, 5])
    p = str(tmp_path / "recount.tsv")
    recruit.write_recount(p, ["7", "21"], counts)
    assert open(p).read() == ("consensus\treads_clustered\treads_recruited\tfrom_own_clusters\tfrom_other_centres\tfrom_unclustered\n"
                              "7\t12\t2\t0\t2\t0\n21\t5\t2\t0\t1\t1\n#ambiguous\t1\n#unassigned\t1\n")
    pa = str(tmp_path / "recount_all.tsv")
    recruit.write_recount(pa, ["7", "21"], counts, sample="s1")
    recruit.write_recount(pa, [], dict(centres=[], ambiguous=0, unassigned=4), sample="s2", header=False, mode="a")
    lines = open(pa).read().splitlines()
    assert lines[0].split("\t")[:2] == ["sample", "consensus"] and lines[1] == "s1\t7\t12\t2\t0\t2\t0" and lines[-2:] == ["#ambiguous\ts2\t0", "#unassigned\ts2\t4"]
    q = str(tmp_path / "read_assignments.tsv")
    recruit.write_assignments(q, ["r%d" % i for i in range(6)], HITS, st, ["7", "21"], [100, 50])
    rows = [l.split("\t") for l in open(q).read().splitlines()]
    assert rows[0] == ["read", "consensus", "strand", "ed", "identity", "status"]
    assert rows[1] == ["r0", "7", "+", "3", "0.9700", "ambiguous"] and rows[2] == ["r1", "21", "-", "2", "0.9600", "assigned"]
    assert rows[5] == ["r4", "-", "-", "-", "-", "unassigned"] and rows[6] == ["r5", "7", "-", "7", "0.9300", "assigned"] and len(rows) == 7


def test_a_library_without_the_kernel_is_an_error(oracle):
    from ngspeciesid_amd._capi import NgsidError
    with pytest.raises(NgsidError):
        oracle.recruit(ReadSet.from_strings(["ACGT"]), [0, 1], ["AC"], [0, 1], [0])


def test_header_declares_and_library_exports_the_call():
    text = open(os.path.join(ROOT, "include", "ngsid_recruit.h")).read()
    assert re.search(r"int32_t\s+ngsid_recruit\s*\(", text) and "NGSID_RECRUIT_MAX_LEN 2048" in text and "NGSID_RECRUIT_NFIELD  6" in text
    from ngspeciesid_amd import runtime
    lib = runtime.load_library()
    assert hasattr(lib, "ngsid_recruit") and lib.ngsid_abi_version() == 2
