"""CPU: the definition of ngsid_error_profile (tests/errprof_reference.py) gives the hand-written tables of tests/errprof_cases.py and keeps the identities
include/ngsid_errprof.h promises against the definitions of ngsid_consensus_support and ngsid_read_cigars; the step logic of k_errprof in Python integers
(tests/errprof_wave_model.py) equals it on rows that cross a 64-position step in every way; and the policy module (ngspeciesid_amd/errprof.py) on hand tables."""
import numpy as np
import pytest
from ngspeciesid_amd import errprof, synth
from ngspeciesid_amd._capi import ReadSet
from support_reference import ed_ops, support_reference
from cigar_reference import cigar_reference, counted
from errprof_reference import errprof_reference, profile_columns, run_lengths, check_identities, NCOUNT, NQ, PAIR, INS_LETTER, CEN_OTHER, READS, INS_LEN, DEL_LEN, HPCTX
import errprof_cases as ec
import errprof_wave_model as em
from cigar_wave_model import rows_of_columns


def _enc(s):
    return np.frombuffer(s.encode(), dtype=np.uint8)


def _names(t):
    """the non-zero cells of a [96] table, for a readable failure"""
    return {int(i): int(t[i]) for i in np.nonzero(t)[0]}


# ---- the definition
def test_flanks_hold_no_run():
    for c in ec.HAND:
        rl = run_lengths(_enc(c["centre"]))
        assert (rl[:40] == 1).all() and (rl[-40:] == 1).all(), c["name"]


@pytest.mark.parametrize("clip", [False, True])
def test_hand_cases_through_the_reference(oracle, clip):
    centres, reads, quals, grp_off, strand = ec.hand_sets()
    counts, qtab, st = errprof_reference(oracle, centres, ReadSet.from_strings(reads, quals), grp_off, clip=clip)
    exp_c, exp_q = ec.hand_expected(clip)
    assert st.tolist() == strand
    for g, c in enumerate(ec.HAND):
        for s in (0, 1):
            assert np.array_equal(counts[g, s], exp_c[g, s]), "%s, strand %d: reference %s, by hand %s" % (c["name"], s, _names(counts[g, s]), _names(exp_c[g, s]))
            assert np.array_equal(qtab[g, s], exp_q[g, s]), "%s, strand %d: qtab" % (c["name"], s)
    assert counts.dtype == np.uint64 and qtab.dtype == np.uint64 and counts.shape == (len(ec.HAND), 2, NCOUNT) and qtab.shape == (len(ec.HAND), 2, NQ, 3)
    # the cases say what they are there for
    by = {c["name"]: g for g, c in enumerate(ec.HAND)}
    g = by["minus_strand_quality_ramp"]
    assert qtab[g, 1, 42, 1] == 1 and qtab[g, 1, 41, 1] == 0 and qtab[g, 0].sum() == 0
    assert counts[by["insertion_behind_the_last_counted_column"], 0, INS_LEN:INS_LEN + 16].sum() == 0
    assert (counts[by["clip"], 0, PAIR:PAIR + 24].sum() == 43) == clip
    none, q_none, _ = errprof_reference(oracle, centres, ReadSet.from_strings(reads), grp_off, clip=clip)          # FASTA reads: the same counts, an all-zero qtab
    assert np.array_equal(none, counts) and q_none.sum() == 0
    assert errprof_reference(oracle, centres, ReadSet.from_strings(reads, quals), grp_off, clip=clip, qualities=False)[1] is None


def _bulk(n=300, mu=14.0, seed=5):
    sp = synth.make_species(2, 300, 0.2, seed=seed)
    rd = synth.make_reads(sp, n, mu=mu, seed=seed + 1, rc_fraction=0.5)
    rs = ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64))
    species = rd["species"].numpy()
    lists = [np.nonzero(species == g)[0].astype(np.uint32) for g in range(2)]
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
    return [s.tobytes().decode() for s in sp], rs, off, np.concatenate(lists)


@pytest.mark.parametrize("clip", [False, True])
def test_identities_against_support_and_cigars(oracle, clip):
    centres, rs, off, ro = _bulk()
    counts, qtab, st = errprof_reference(oracle, centres, rs, off, ro, clip=clip)
    sup, cen_off, used, st2 = support_reference(oracle, centres, rs, off, ro, clip=clip)
    aln, _, _, st3 = cigar_reference(oracle, centres, rs, off, ro, clip=clip)
    assert np.array_equal(st, st2) and np.array_equal(st, st3) and (st == 0).sum() > 50 and (st == 1).sum() > 50
    check_identities(counts, qtab, sup, cen_off, used, aln, off)
    assert counts[:, :, INS_LEN:INS_LEN + 16].sum() > 100 and counts[:, :, DEL_LEN:DEL_LEN + 16].sum() > 100 and counts[:, :, HPCTX + 4:HPCTX + 32].sum() > 1000


# ---- the step logic of the kernel
def _pair_of_body(rng, m, t0, body, lead=0, trail=0, runs=True):
    """a centre of m letters (with runs of equal letters), and the read, its qualities and the oracle-style column list of `body` (over = X I D) placed at centre position t0
    with `lead` / `trail` free read letters"""
    centre = []
    while len(centre) < m: centre += ["ACGT"[int(rng.integers(4))]] * (int(rng.integers(1, 12)) if runs and rng.random() < 0.3 else 1)
    centre = "".join(centre[:m])
    if m > 20: centre = centre[:17] + "N" + centre[18:]
    other = lambda c: "N" if rng.random() < 0.2 else "ACGT"[("ACGT".find(c) + 1) % 4]
    read, ti = ["T"] * lead, t0
    for c in body:
        if c == "=": read.append(centre[ti] if centre[ti] != "N" else "A"); ti += 1
        elif c == "X": read.append(other(centre[ti])); ti += 1
        elif c == "I": read.append("GN"[int(rng.random() < 0.2)])
        else: ti += 1
    assert ti <= m
    read += ["C"] * trail
    cols = [3] * t0 + [2] * lead + ["=XID".index(c) for c in body] + [2] * trail + [3] * (m - ti)
    cols = np.array(cols, dtype=np.uint8)
    at_n = [x for x in np.nonzero(cols == 0)[0] if centre[int((cols[:x] != 2).sum())] == "N"]      # a base opposite the centre's N is a mismatch column
    cols[at_n] = 1
    qual = rng.integers(20, 127, size=len(read)).astype(np.uint8)
    return cols, "".join(read), qual, centre


STEP_CASES = [
    # (centre length, t_begin, body, lead, trail)
    (7, 0, "=" * 7, 0, 0), (8, 0, "=" * 8, 0, 0), (9, 0, "=" * 9, 0, 0), (63, 0, "=" * 63, 0, 0), (64, 0, "=" * 64, 0, 0), (65, 0, "=" * 65, 0, 0), (129, 0, "=" * 129, 0, 0),
    (129, 0, "=" * 62 + "DDD" + "=" * 64, 0, 0), (129, 0, "=" * 63 + "DD" + "=" * 64, 0, 0),           # a 'D' run over 63 | 64
    (129, 0, "=" * 63 + "D" + "=" * 65, 0, 0), (129, 0, "=" * 62 + "DD" + "=" * 65, 0, 0),             # ... ending at 63: lane 0 of the next step closes it
    (129, 0, "=" * 64 + "D" + "=" * 64, 0, 0), (129, 0, "=" * 64 + "D" * 17 + "=" * 48, 0, 0),         # ... beginning at 64; 16+
    (200, 0, "=" * 126 + "DDDD" + "=" * 70, 0, 0), (200, 0, "=" * 60 + "D" * 70 + "=" * 70, 0, 0),     # over 127 | 128; over a whole step
    (200, 0, "=" * 60 + "D" * 68 + "=" * 72, 0, 0), (200, 3, "=" + "D" * 140 + "=", 0, 0),             # ... ending at 127; over two boundaries
    (129, 0, "=" * 63 + "XX" + "=" * 64, 2, 3), (129, 0, "=" * 64 + "X" * 64 + "=", 0, 0),             # 'X' over the boundary, a whole step of 'X'
    (130, 0, "=" * 64 + "I" + "=" * 66, 0, 0), (130, 0, "=" * 64 + "III" + "X" + "=" * 65, 0, 0),      # an insertion behind position 63
    (130, 0, "=" * 65 + "I" * 16 + "=" * 65, 0, 0), (130, 0, "=" * 63 + "I" * 40 + "=" * 67, 0, 0),    # ... behind 64, behind 62: 16+
    (130, 0, "=" * 128 + "I" + "==", 0, 0), (130, 0, "=" * 63 + "X" + "I" * 15 + "X" + "=" * 65, 0, 0),
    (100, 0, "=" * 98 + "II" + "=", 0, 0), (65, 0, "=" * 63 + "I" + "=", 0, 4),                        # ... behind t_end - 1 (with t_end = 64: across the step)
    (129, 1, "=" * 100, 0, 0), (129, 7, "=X" * 50, 3, 0), (129, 8, "=" * 121, 0, 5), (129, 63, "=" * 66, 5, 0), (129, 63, "=D" + "=" * 10, 1, 1),      # spans that begin inside a dword / a step
    (129, 64, "=I=D=X=", 0, 0), (200, 60, "X" + "=" * 3 + "D" + "=" * 70 + "I" + "X=", 9, 9),
    (80, 10, "=" * 30, 0, 6), (129, 0, "=" * 64, 0, 2), (129, 0, "=" * 128, 0, 2),                     # a flag on t_end itself (trailing read letters): not counted
    (70, 5, "=", 4, 4), (70, 63, "X", 0, 3), (70, 64, "=", 2, 0), (1, 0, "=", 0, 0),                   # a one-column span
]


def _model_equals_reference(cols, read, qual, centre, clip):
    cnt = np.zeros(NCOUNT, dtype=np.uint64); qt = np.zeros((NQ, 3), dtype=np.uint64)
    profile_columns(cnt, qt, cols, _enc(read), qual, _enc(centre), clip)
    c = counted(cols, clip)
    span = (-1, -1, -1, -1)
    if c is not None:
        in_q = cols != 3; in_t = cols != 2
        qi = np.cumsum(in_q) - in_q; ti = np.cumsum(in_t) - in_t
        span = (int(qi[c[0]]), int(qi[c[1]]), int(ti[c[0]]), int(ti[c[1]]))
    nib, pos = rows_of_columns(cols, _enc(read), len(centre))
    got_c, got_q = em.walk(nib, pos, span, _enc(read), qual, _enc(centre))
    assert got_c == cnt.tolist(), "model %s, reference %s" % (_names(np.array(got_c)), _names(cnt))
    assert got_q == qt.tolist()
    no_q = em.walk(nib, pos, span, _enc(read), None, _enc(centre))
    assert no_q[0] == got_c and sum(map(sum, no_q[1])) == 0
    return cnt


@pytest.mark.parametrize("case", range(len(STEP_CASES)))
def test_wave_model_equals_reference_across_steps(case):
    m, t0, body, lead, trail = STEP_CASES[case]
    cols, read, qual, centre = _pair_of_body(np.random.default_rng(500 + case), m, t0, body, lead, trail)
    cnt = _model_equals_reference(cols, read, qual, centre, False)
    assert cnt[READS] == 1 and cnt[INS_LEN:INS_LEN + 16].sum() == sum(1 for a, b in zip(body[:-1], body[1:]) if a != "I" and b == "I")


def test_wave_model_equals_reference_on_random_pairs(oracle):
    rng = np.random.default_rng(2027)
    seen = 0
    for x in range(200):
        m = int(rng.integers(1, 201)); err = float(rng.uniform(0.0, 0.4))
        centre = "".join("ACGT"[v] * (int(rng.integers(2, 12)) if rng.random() < 0.1 else 1) for v in rng.integers(4, size=m))[:m]
        body = []
        for c in centre:
            u = rng.random()
            if u < err / 3: continue
            if u < 2 * err / 3: body.append("ACGTN"[int(rng.integers(5))]); continue
            body.append(c)
            if u > 1 - err / 3: body.append("ACGT"[int(rng.integers(4))] * int(rng.integers(1, 4)))
        read = "GATTACA"[:int(rng.integers(0, 8))] + "".join(body) + "CCTGA"[:int(rng.integers(0, 6))] or "A"
        cols = ed_ops(oracle, _enc(read), _enc(centre))
        qual = rng.integers(30, 90, size=len(read)).astype(np.uint8)
        for clip in (False, True):
            seen += int(_model_equals_reference(cols, read, qual, centre, clip)[READS])
    assert seen > 250


# ---- the policy module
def _hand_table():
    t = np.zeros((2, NCOUNT), dtype=np.uint64)
    t[0, PAIR + 0 * 6 + 0] = 900; t[0, PAIR + 1 * 6 + 1] = 50; t[0, PAIR + 0 * 6 + 2] = 30; t[0, PAIR + 0 * 6 + 5] = 20      # strand 0: 1000 aligned, 30 A>G, 20 A deleted
    t[0, INS_LETTER + 3] = 10; t[0, INS_LEN + 0] = 6; t[0, INS_LEN + 1] = 2; t[0, DEL_LEN + 0] = 20; t[0, READS] = 4
    t[1, PAIR + 3 * 6 + 3] = 990; t[1, PAIR + 3 * 6 + 1] = 10; t[1, READS] = 5                                                 # strand 1: 1000 aligned, 10 T>C
    t[0, HPCTX + 0 * 4 + 0] = 900; t[0, HPCTX + 0 * 4 + 1] = 30; t[0, HPCTX + 2 * 4 + 0] = 50; t[0, HPCTX + 2 * 4 + 2] = 20; t[0, HPCTX + 2 * 4 + 3] = 7
    return t


def test_rates_spectrum_lengths_and_hp_table():
    t = _hand_table()
    r = errprof.rates(t)
    assert r["0"] == dict(aligned=1000.0, substitution=0.03, insertion=0.01, deletion=0.02, total=pytest.approx(0.06))
    assert r["1"]["substitution"] == 0.01 and r["1"]["insertion"] == 0.0 and r["1"]["deletion"] == 0.0
    assert r["both"]["aligned"] == 2000.0 and r["both"]["substitution"] == 0.02 and r["both"]["deletion"] == 0.01 and r["both"]["insertion"] == 0.005
    assert errprof.rates(np.stack([t, t]))["both"] == dict(r["both"], aligned=4000.0)          # groups are summed
    s = errprof.spectrum(t)
    assert s.shape == (4, 4) and s[0, 2] == 0.75 and s[3, 1] == 0.25 and s.sum() == 1.0 and np.trace(s) == 0.0
    il = errprof.indel_lengths(t)
    assert il["ins"].tolist() == [6, 2] + [0] * 14 and il["dele"][0] == 20 and il["ins_share"][0] == 0.75 and il["del_share"][0] == 1.0
    h = errprof.hp_table(t)
    assert h["n"].tolist() == [930, 0, 70, 0, 0, 0, 0, 0] and h["sub"][0] == 30 / 930 and h["dele"][2] == 20 / 70 and h["ins_behind"][2] == 0.1 and h["sub"][1] == 0.0
    su = errprof.summary(t)
    assert su["bases"] == 1990 and su["errors"] == 50 and su["error_rate"] == 50 / 1990 and su["phred"] == pytest.approx(-10 * np.log10(50 / 1990)) and su["reported_error"] is None


def test_all_zero_tables():
    z = np.zeros((3, 2, NCOUNT), dtype=np.uint64)
    r = errprof.rates(z)
    assert all(r[s] == dict(aligned=0.0, substitution=0.0, insertion=0.0, deletion=0.0, total=0.0) for s in errprof.STRANDS)
    assert errprof.spectrum(z).sum() == 0 and errprof.hp_table(z)["sub"].sum() == 0 and errprof.indel_lengths(z)["ins_share"].sum() == 0
    su = errprof.summary(z, np.zeros((3, 2, NQ, 3), dtype=np.uint64))
    assert su["error_rate"] == 0.0 and su["phred"] is None and su["reported_error"] is None
    assert len(errprof.calibration(np.zeros((2, NQ, 3), dtype=np.uint64))["q"]) == 0
    assert len(errprof.calibration(np.zeros((2, NQ, 3), dtype=np.uint64), min_obs=0)["q"]) == 0          # no base, no row


def test_calibration_min_obs_and_pseudo_count():
    q = np.zeros((2, NQ, 3), dtype=np.uint64)
    q[0, 10] = (880, 60, 20); q[1, 10] = (18, 20, 0)          # q 10: 998 bases, 100 errors
    q[0, 30] = (98, 0, 0)                                      # q 30: 98 bases, no error
    q[1, 50] = (3, 1, 0)
    c = errprof.calibration(q, min_obs=50)
    assert c["q"].tolist() == [10, 30] and c["n_match"].tolist() == [898, 98] and c["n_sub"].tolist() == [80, 0] and c["n_ins"].tolist() == [20, 0]
    assert c["empirical_q"][0] == pytest.approx(-10 * np.log10(101 / 1000)) and c["empirical_q"][1] == pytest.approx(20.0)      # (0 + 1) / (98 + 2): finite without an error
    assert errprof.calibration(q, min_obs=99)["q"].tolist() == [10] and errprof.calibration(q, min_obs=1)["q"].tolist() == [10, 30, 50]
    assert errprof.calibration(q)["q"].tolist() == [10] and errprof.MIN_OBS == 100
    su = errprof.summary(_hand_table(), q)
    n = np.array([998, 98, 4]); rep = (n * 10.0 ** (-np.array([10, 30, 50]) / 10.0)).sum() / n.sum()
    assert su["reported_error"] == pytest.approx(rep) and su["reported_phred"] == pytest.approx(-10 * np.log10(rep))


def test_writer_round_trip(tmp_path):
    t = _hand_table(); u = np.zeros((2, NCOUNT), dtype=np.uint64); u[1, READS] = 1; u[1, HPCTX + 31] = 3; u[1, DEL_LEN + 15] = 2; u[0, CEN_OTHER] = 9; u[0, INS_LETTER + 4] = 1
    path = str(tmp_path / "error_profile.tsv")
    errprof.write(path, [("7", t), ("12", u)])
    back = errprof.read_table(path)
    assert sorted(back["counts"]) == ["12", "7"] and np.array_equal(back["counts"]["7"], t) and np.array_equal(back["counts"]["12"], u)
    assert back["rates"]["7"]["0"]["substitution"] == 0.03 and back["rates"]["7"]["both"] == errprof.rates(t)["both"] and back["rates"]["12"]["1"]["total"] == 0.0
    lines = open(path).read().split("\n")
    assert lines[0].split("\t") == list(errprof.TABLE_HEADER) and "" in lines and lines[lines.index("") + 1].split("\t") == list(errprof.RATE_HEADER)
    assert "7\t0\tPAIR\tA\tG\t30" in lines and "12\t1\tHPCTX\t8+\tins_behind\t3" in lines and "12\t1\tDEL_LEN\t-\t16+\t2" in lines and "12\t0\tREADS\t-\t-\t0" in lines
    q = np.zeros((2, NQ, 3), dtype=np.uint64); q[0, 10] = (880, 60, 20); q[1, 93] = (200, 0, 0)
    cpath = str(tmp_path / "quality_calibration.tsv")
    errprof.write_calibration(cpath, q)
    c = errprof.read_calibration(cpath)
    assert open(cpath).readline().rstrip("\n").split("\t") == list(errprof.CALIBRATION_HEADER)
    assert c["q"].tolist() == [10, 93] and c["n_match"].tolist() == [880, 200] and c["n_sub"].tolist() == [60, 0] and c["n_ins"].tolist() == [20, 0]
    assert c["empirical_q"] == pytest.approx(errprof.calibration(q)["empirical_q"], abs=1e-3)
    # with a sample in front, appended
    errprof.write(path, [("7", t)], sample="s1"); errprof.write(path, [("12", u)], sample="s2", header=False, mode="a")
    rows = [l.split("\t") for l in open(path).read().split("\n") if l]
    assert rows[0] == ["sample"] + list(errprof.TABLE_HEADER) and {r[0] for r in rows[1:] if r[0] != "sample"} == {"s1", "s2"}
