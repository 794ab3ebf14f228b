"""CPU: tests/chimera_reference.py (the definition of include/ngsid_chimera.h in numpy) against a scalar restatement without numpy, hand anchors, and the policy
layer ngspeciesid_amd/chimera.py (candidates, call, the table, the flags)."""
import argparse
import numpy as np
import pytest
import chimera_reference as ref
import chimera_cases as cases
from ngspeciesid_amd import chimera, classify
from ngspeciesid_amd._capi import ReadSet, CHIMERA_FIELDS, CHIMERA_NFIELD, CHIMERA_ROWS, CHIMERA_STRIP, chimera_profile_offsets


# ---- the definition once more, cell by cell
def _ed_table(q, p):
    D = [[0] * (len(p) + 1) for _ in range(len(q) + 1)]
    for i in range(len(q) + 1):
        for j in range(len(p) + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
            else:
                D[i][j] = min(D[i - 1][j - 1] + (q[i - 1] != p[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return D


def _scalar_profiles(q, p):
    n = len(q)
    F = [min(row) for row in _ed_table(q, p)]
    back = [min(row) for row in _ed_table(q[::-1], p[::-1])]
    return F, [back[n - i] for i in range(n + 1)]


def _scalar_model(queries, parents, pair_off, pair_parent, gid):
    fields, prof = [], []
    for qi, q in enumerate(queries):
        n = len(q)
        ks = list(range(pair_off[qi], pair_off[qi + 1]))
        FB = [_scalar_profiles(q, parents[pair_parent[k]]) for k in ks]
        for F, B in FB: prof += F + B
        row = [-1] * 7
        if ks:
            row[1] = min(F[n] for F, _ in FB)
            row[0] = min(x for x, (F, _) in enumerate(FB) if F[n] == row[1])
            admissible = [(a, b) for a in range(len(ks)) for b in range(len(ks)) if gid[ks[a]] != gid[ks[b]]]
            if admissible:
                two = min(FB[a][0][i] + FB[b][1][i] for a, b in admissible for i in range(n + 1))
                lo = min(i for a, b in admissible for i in range(n + 1) if FB[a][0][i] + FB[b][1][i] == two)
                pa, pb = min((a, b) for a, b in admissible if FB[a][0][lo] + FB[b][1][lo] == two)
                hi = max(i for i in range(n + 1) if FB[pa][0][i] + FB[pb][1][i] == two)
                row[2:] = [two, pa, pb, lo, hi]
        fields.append(row)
    return fields, prof


@pytest.mark.parametrize("seed", range(4))
def test_reference_equals_the_scalar_restatement(seed):
    rng = np.random.default_rng(40 + seed)
    queries, parents, pair_off, pair_parent, gid = cases.random_small(rng, 150)
    for g in (gid, None):
        fields, prof, prof_off = ref.chimera_model(queries, parents, pair_off, pair_parent, g)
        want_f, want_p = _scalar_model(queries, parents, pair_off, pair_parent, pair_parent if g is None else g.tolist())
        assert fields.dtype == np.int32 and prof.dtype == np.uint16 and fields.tolist() == want_f and prof.tolist() == want_p
        assert np.array_equal(prof_off, chimera_profile_offsets([len(q) for q in queries], pair_off))
    f = fields if gid is None else ref.chimera_model(queries, parents, pair_off, pair_parent, gid)[0]
    has = f[:, 2] >= 0
    assert has.any() and (~has).any() and (f[has, 1] >= f[has, 2]).all()            # the gain is never negative
    assert (f[has, 5] <= f[has, 6]).all()


def test_hand_anchors():
    A, B = "A" * 20, "C" * 20
    for k in range(1, 20):
        f = ref.chimera_model([A[:k] + B[k:]], [A, B], [0, 2], [0, 1])[0][0].tolist()
        assert f[2:] == [0, 0, 1, k, k] and f[1] == min(k, 20 - k) and f[0] == (0 if k >= 10 else 1)
    # the ends: everything from one parent; the smallest i and then the smallest pair decide
    assert ref.chimera_model([B], [A, B], [0, 2], [0, 1])[0][0].tolist() == [1, 0, 0, 0, 1, 0, 0]
    assert ref.chimera_model([A], [A, B], [0, 2], [0, 1])[0][0].tolist() == [0, 0, 0, 1, 0, 0, 0]
    assert ref.chimera_model([A], [A, B], [0, 2], [0, 1], [7, 7])[0][0].tolist() == [0, 0, -1, -1, -1, -1, -1]      # both pairs of one gid
    assert ref.chimera_model([A, B], [A, B], [0, 0, 1], [1])[0].tolist() == [[-1] * 7, [0, 0, -1, -1, -1, -1, -1]]   # no pair; one pair
    F, Bk = ref.profiles_of("ACGT", "AGT")
    assert F.tolist() == [0, 0, 1, 1, 1] and Bk.tolist() == [1, 1, 0, 0, 0]
    F, Bk = ref.profiles_of("ACGT", "")
    assert F.tolist() == [0, 1, 2, 3, 4] and Bk.tolist() == [4, 3, 2, 1, 0]
    F, Bk = ref.profiles_of("", "ACGT")
    assert F.tolist() == [0] and Bk.tolist() == [0]
    assert ref.profiles_of("ANNA", "ANCA")[0].tolist() == [0, 0, 0, 1, 1]            # N equals only N


def test_constants():
    assert CHIMERA_FIELDS == ("one_pair", "one_cost", "two_cost", "pair_a", "pair_b", "bp_lo", "bp_hi") and CHIMERA_NFIELD == ref.NFIELD == 7 and CHIMERA_STRIP == 64 * CHIMERA_ROWS


# ---- policy
def test_candidates_at_the_abundance_skew_border():
    off, parent, gid = chimera.candidates([20, 10, 9, 11, 40], 2.0)
    rows = [parent[int(off[q]):int(off[q + 1])].tolist() for q in range(5)]
    assert rows == [[8, 9], [0, 1, 8, 9], [0, 1, 8, 9], [8, 9], []]                  # 20 >= 2 * 10 offers, 20 >= 2 * 11 does not
    assert gid.tolist() == [p // 2 for p in parent.tolist()]                         # both strands of a parent share its gid
    off, parent, gid = chimera.candidates([5, 5], 1.0)
    assert parent.tolist() == [2, 3, 0, 1] and off.tolist() == [0, 2, 4]             # never its own parent
    off, parent, gid = chimera.candidates([], 2.0)
    assert off.tolist() == [0] and len(parent) == 0 and parent.dtype == np.uint32 and gid.dtype == np.int32 and off.dtype == np.uint64


def test_both_strands_share_a_gid_and_find_a_reversed_parent():
    rng = np.random.default_rng(3)
    a, b = cases.family(rng, 2, 60, 0.4)
    q = a[:30] + b[30:]
    seqs = [classify.both_strands(ReadSet.from_strings([a])).get(1)[0], b, q]        # a is in the other orientation
    fields, off, parent, gid = chimera.model(_RefApi(), seqs, np.array([50, 40, 5]))
    d = chimera.describe(fields, off, parent, [len(s) for s in seqs], chimera.call(fields, [len(s) for s in seqs]))
    assert [x["chimeric"] for x in d] == [False, False, True]
    assert (d[2]["parent_a"], d[2]["strand_a"], d[2]["parent_b"], d[2]["strand_b"], d[2]["model_ed"]) == (0, 1, 1, 0, 0) and d[2]["bp_lo"] <= 30 <= d[2]["bp_hi"]
    assert d[0]["best_parent"] == -1 and d[0]["model_ed"] == -1 and d[0]["gain"] == -1 and d[1]["best_parent"] == -1


class _RefApi:
    """Api.chimera_model answered by the numpy reference"""

    def chimera_model(self, queries, parents, pair_off, pair_parent, pair_gid=None, profiles=False):
        strs = lambda rs: [rs.get(i)[0] for i in range(rs.n)] if isinstance(rs, ReadSet) else list(rs)
        f, p, o = ref.chimera_model(strs(queries), strs(parents), pair_off, pair_parent, pair_gid)
        return (f, p, o) if profiles else f


def test_call_at_each_threshold():
    assert (chimera.DEFAULTS["min_gain"], chimera.DEFAULTS["max_model_frac"]) == (5, 0.005)      # tools/chimera_sweep.py, profiles/chimera.txt
    n = 600
    base = [0, 8, 3, 0, 2, 100, 140]                                                  # gain 5, model 3 = 0.005 * 600
    assert chimera.call([base], [n]).tolist() == [True]
    for change, length in (({1: 7}, n), ({2: 4, 1: 9}, n), ({}, 599), ({5: 0}, n), ({6: n}, n), ({2: -1, 3: -1, 4: -1, 5: -1, 6: -1}, n)):
        f = list(base)
        for k, v in change.items(): f[k] = v
        assert chimera.call([f], [length]).tolist() == [False], change
    assert chimera.call([base], [n], min_gain=6).tolist() == [False] and chimera.call([[0, 7, 3, 0, 2, 100, 140]], [n], min_gain=4).tolist() == [True]
    assert chimera.call([[0, 9, 4, 0, 2, 100, 140]], [n], max_model_frac=0.01).tolist() == [True]
    assert chimera.call([[0, 8, 3, 0, 2, 1, n - 1]], [n]).tolist() == [True]         # a breakpoint one base from either end is inside
    assert chimera.call(np.zeros((0, 7), np.int32), []).tolist() == []


def test_table_round_trip(tmp_path):
    ids = ["consensus_cl_id_3_total_supporting_reads_50", "consensus_cl_id_9_total_supporting_reads_40", "consensus_cl_id_1_total_supporting_reads_5"]
    assert [classify.n_reads_of(i) for i in ids] == [50, 40, 5]
    entries = [dict(chimeric=False, length=600, best_parent=-1, best_strand=-1, best_ed=-1, parent_a=-1, strand_a=-1, parent_b=-1, strand_b=-1, model_ed=-1, gain=-1, bp_lo=-1, bp_hi=-1),
               dict(chimeric=False, length=601, best_parent=0, best_strand=0, best_ed=70, parent_a=-1, strand_a=-1, parent_b=-1, strand_b=-1, model_ed=-1, gain=-1, bp_lo=-1, bp_hi=-1),
               dict(chimeric=True, length=598, best_parent=1, best_strand=1, best_ed=31, parent_a=0, strand_a=0, parent_b=1, strand_b=1, model_ed=1, gain=30, bp_lo=290, bp_hi=304)]
    rows = chimera.table_rows(ids, [50, 40, 5], entries)
    assert rows[2]["parent_a"] == ids[0] and rows[2]["strand_b"] == "-" and rows[0]["best_parent"] == "*" and rows[0]["best_strand"] == "*"
    path = str(tmp_path / "chimeras.tsv")
    chimera.write_table(path, rows)
    assert open(path).readline() == "#" + "\t".join(chimera.COLUMNS) + "\n" and chimera.read_table(path) == rows
    with_sample = chimera.table_rows(ids, [50, 40, 5], entries, sample="s1")
    chimera.write_table(path, with_sample, with_sample=True)
    assert open(path).readline().startswith("#sample\tid\t") and chimera.read_table(path) == with_sample
    assert chimera.COLUMNS == ("id", "n_reads", "length", "chimeric", "best_parent", "best_strand", "best_ed", "parent_a", "strand_a", "parent_b", "strand_b", "model_ed", "gain", "bp_lo", "bp_hi")


def test_run_writes_one_table_per_group(tmp_path):
    rng = np.random.default_rng(5)
    a, b, c = cases.family(rng, 3, 80, 0.4)
    q = a[:40] + b[40:]
    name = "consensus_cl_id_%d_total_supporting_reads_%d"
    g1 = [(name % (0, 50), 50, a), (name % (4, 40), 40, b), (name % (7, 6), 6, q)]
    g2 = [(name % (2, 9), 9, c), (name % (3, 3), 3, q)]                             # q's parents are in the OTHER sample: no model from them
    for s in ("s1", "s2"): (tmp_path / s).mkdir()
    args = argparse.Namespace(outfolder=str(tmp_path), **{"chimera_" + k: v for k, v in chimera.DEFAULTS.items()})
    rows = chimera.run(args, _RefApi(), [("s1", str(tmp_path / "s1"), g1), ("s2", str(tmp_path / "s2"), g2)])
    assert [r["chimeric"] for r in rows[0]] == [0, 0, 1] and [r["chimeric"] for r in rows[1]] == [0, 0]
    assert rows[0][2]["parent_a"] == g1[0][0] and rows[0][2]["parent_b"] == g1[1][0] and rows[1][1]["best_parent"] == g2[0][0] and rows[1][1]["parent_a"] == "*"
    plain = lambda rs: [{k: v for k, v in r.items() if k != "sample"} for r in rs]          # the sample column is in chimeras_all.tsv only
    assert chimera.read_table(str(tmp_path / "s1" / "chimeras.tsv")) == plain(rows[0]) and chimera.read_table(str(tmp_path / "s2" / "chimeras.tsv")) == plain(rows[1])
    assert chimera.read_table(str(tmp_path / "chimeras_all.tsv")) == [dict(r) for r in rows[0] + rows[1]]


def test_check_args_and_flags():
    from ngspeciesid_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["--fastq", "x"])
    assert a.chimeras is False and (a.chimera_min_abskew, a.chimera_min_gain, a.chimera_max_model_frac) == tuple(chimera.DEFAULTS[k] for k in ("min_abskew", "min_gain", "max_model_frac"))
    assert chimera.check_args(a) is None and chimera.DEFAULTS["min_abskew"] == 2.0
    for flag, val in (("--chimera_min_abskew", "0"), ("--chimera_min_gain", "0"), ("--chimera_max_model_frac", "1.5"), ("--chimera_max_model_frac", "-0.1")):
        assert chimera.check_args(p.parse_args(["--fastq", "x", "--chimeras", flag, val])), flag
    sub = cli._chimeras_subparser(argparse.ArgumentParser()).parse_args(["--fasta", "f", "--outfile", "o", "--chimera_min_gain", "5"])
    assert sub.which == "chimeras" and sub.chimera_min_gain == 5 and chimera.check_args(sub) is None
    with pytest.raises(SystemExit):
        cli.cli(["--fastq", "x", "--chimeras"])                                     # needs --consensus
