"""CPU: the policy layer of the reference-library search (ngspeciesid_amd/classify.py) and the test reference itself (tests/classify_reference.py over the oracle's
minimizer call) against a scalar restatement of the definition in include/ngsid_classify.h."""
import itertools
import numpy as np
import pytest
import classify_reference as ref
from ngspeciesid_amd import classify


# ---- scalar restatement: minimizers of the homopolymer-compressed string as Python strings (the window rule of cluster.get_kmer_minimizers: w - k + 1 consecutive
# k-mers per window, slices past the end are shorter strings and compare as such; the minimum is looked for again when the k-mer that leaves the window EQUALS it,
# otherwise a new k-mer takes over only when it is smaller), sets of strings, plain loops
def _hpc(s):
    return "".join(ch for ch, _ in itertools.groupby(s))


def _scalar_set(seq, k, w):
    s = _hpc(seq)
    if len(s) < k:
        return set()
    span = w - k + 1
    window = [s[i:i + k] for i in range(span)]
    cur = min(window); chosen = {cur}
    for i in range(span, len(s) - k + 1):
        gone = window.pop(0); window.append(s[i:i + k])
        if gone == cur:
            cur = min(window); chosen.add(cur)
        elif window[-1] < cur:
            cur = window[-1]; chosen.add(cur)
    return chosen


def _scalar_search(refs, queries, k, w, top_k, min_shared):
    rsets = [_scalar_set(r, k, w) for r in refs]
    rows = []
    for q in queries:
        f, r = _scalar_set(q, k, w), _scalar_set(ref.revcomp(q), k, w)
        cands = []
        for x, rs in enumerate(rsets):
            a, b = len(f & rs), len(r & rs)
            sh, st = (b, 1) if b > a else (a, 0)
            if sh >= min_shared:
                cands.append((-sh, x, st))
        cands.sort()
        rows.append(([c[1] for c in cands[:top_k]], [-c[0] for c in cands[:top_k]], [c[2] for c in cands[:top_k]], [len(f), len(r)]))
    return rows


def _compare(oracle, refs, queries, k, w, top_k, min_shared):
    got = ref.search(oracle, refs, queries, k, w, top_k, min_shared)
    want = _scalar_search(refs, queries, k, w, top_k, min_shared)
    for q, (r, sh, st, nc) in enumerate(want):
        pad = [-1] * (top_k - len(r))
        assert got[0][q].tolist() == r + pad and got[1][q].tolist() == sh + pad and got[2][q].tolist() == st + pad and got[3][q].tolist() == nc, (q, queries[q])
    return got


def test_tandem_repeat_counts_once(oracle):
    """k = 3, w = 5: three 3-mers per window.  q = ACG x 5 (15 bases, no homopolymer run): its 3-mers are ACG CGA GAC ACG ..., 13 of them.  The first window
    (ACG CGA GAC) picks ACG at 0; every time that ACG leaves the window (at 3-mers 3, 6, 9, 12) the minimum is looked for again and is the next ACG: the code ACG is
    returned FIVE times (positions 0 3 6 9 12) and nothing else, so S(q) = {ACG} and n_codes = 1.  The reverse complement CGT x 5 gives S = {CGT}.
    r0 = q has S = {ACG}: shared(q, 0, r0) = 1 (not 5), shared(q, 1, r0) = 0 -> shared 1, strand 0.  r1 = CGT x 5: shared 0 / 1 -> shared 1, strand 1.  r2 = TTGTTG...
    shares nothing.  Order by (shared descending, ref ascending): r0, r1."""
    q = "ACG" * 5
    refs = [q, "CGT" * 5, "TGTGTGTGTGTGTG"]
    assert _scalar_set(q, 3, 5) == {"ACG"} and _scalar_set(ref.revcomp(q), 3, 5) == {"CGT"}
    got = _compare(oracle, refs, [q], 3, 5, 4, 1)
    assert got[0][0].tolist() == [0, 1, -1, -1] and got[1][0].tolist() == [1, 1, -1, -1] and got[2][0].tolist() == [0, 1, -1, -1] and got[3][0].tolist() == [1, 1]


def test_palindrome_ties_and_reports_strand_0(oracle):
    """k = 3, w = 5.  q = ACGTACGT is its own reverse complement.  3-mers: ACG CGT GTA TAC ACG CGT.  First window -> ACG at 0; it leaves at 3-mer 3: the window
    CGT GTA TAC -> CGT; that leaves at 3-mer 4: GTA TAC ACG -> ACG; 3-mer 5 (CGT) is not smaller.  S(q_0) = S(q_1) = {ACG, CGT}.  Against r0 = q both strands share 2:
    a tie, strand 0."""
    q = "ACGTACGT"
    assert ref.revcomp(q) == q and _scalar_set(q, 3, 5) == {"ACG", "CGT"}
    got = _compare(oracle, [q, "GGATCCGGATCC"], [q], 3, 5, 2, 1)
    assert got[0][0, 0] == 0 and got[1][0, 0] == 2 and got[2][0, 0] == 0 and got[3][0].tolist() == [2, 2]


def test_reference_equals_the_scalar_restatement_on_hand_written_cases(oracle):
    a = "ACGTTGCATGCCGATAGGCTTAACGGATCCATGACTGACCTGAAGTCGATCGGATTACAGGCATCGA"
    b = "TTGACCGGTAACGTTAGCATCGGCTAAGGCTTTACGGACTAGGCATTGACCAGTTGACAAGT"
    refs = [a, b, a[:40] + b[20:], ref.revcomp(a), a, "A" * 50, "ACAC" * 20, "", "ACGTNNACGTTGCANNGGATCC" + a[10:50], b[::-1]]
    queries = [a, ref.revcomp(b), a[5:45], a[:30] + "N" + a[31:], "AAAACCCCGGGGTTTT" * 4, "", "ACG", "GT" * 30, b[:25] + a[25:], ref.revcomp(a[:40] + b[20:]), "C" * 40, a[::-1]]
    for k, w in ((3, 5), (5, 8), (7, 7), (13, 20)):
        for top_k, min_shared in ((1, 1), (3, 2), (12, 1)):
            _compare(oracle, refs, queries, k, w, top_k, min_shared)
    got = _compare(oracle, refs, queries, 5, 8, 12, 1)
    assert got[0][0, :2].tolist() == [0, 4] and got[2][0, 0] == 0            # identical references: the smaller index first
    assert got[0][1, 0] == 1 and got[2][1, 0] == 1                          # the reverse complement of b finds b on strand 1
    assert (got[0][5] == -1).all() and got[3][5].tolist() == [0, 0]         # the empty query


TRUTH_SEED = 31      # tests/test_gpu_classify.py uses the same seed and asks the device for 100 % recovery: this is the check that the definition itself recovers all 60


def test_truth_seed_recovers_every_member_with_the_oracle_backend(oracle):
    t = ref.make_truth(TRUTH_SEED, n_members=200, length=400, divergence=0.15, n_queries=60, rate=0.03)
    cand_ref, cand_shared, cand_strand, _ = ref.search(oracle, t["refs"], t["queries"], 13, 20, 8, 3)
    hits = classify.rank(cand_ref, cand_shared, cand_strand, classify.verify(oracle, t["queries"], t["refs"], cand_ref, cand_strand))
    ok = [bool(hs) and hs[0]["ref"] == t["member"][q] and hs[0]["strand"] == t["strand"][q] and hs[0]["called"] for q, hs in enumerate(hits)]
    assert sum(ok) == 60, [q for q, x in enumerate(ok) if not x]


def test_identity_from_columns():
    f = classify.identity_from_columns
    assert f("DDD====IIII") == dict(aln_cols=4, n_match=4, identity=1.0, q_cov=0.5, r_cov=4 / 7)                       # only end gaps
    assert f("IIIDDD") == dict(aln_cols=0, n_match=0, identity=0.0, q_cov=0.0, r_cov=0.0) == f("")                     # no aligned column
    d = f("II===D==I=X=DD")                                                                                           # an interior gap of each kind
    assert d["aln_cols"] == 10 and d["n_match"] == 7 and d["identity"] == 7 / 10 and d["q_cov"] == 9 / 11 and d["r_cov"] == 9 / 11
    d = f("DX===XII")                                                                                                 # an X at either edge is an aligned column
    assert d["aln_cols"] == 5 and d["n_match"] == 3 and d["identity"] == 3 / 5 and d["q_cov"] == 5 / 7 and d["r_cov"] == 5 / 6
    assert f("IDID==")["aln_cols"] == 2 and f("=")["identity"] == 1.0                                                  # a mixed leading run goes as a whole


def test_rank_order_and_called_thresholds():
    cand_ref = np.array([[7, 3, 9, 5, -1]]); cand_shared = np.array([[40, 30, 30, 30, -1]]); cand_strand = np.array([[0, 1, 0, 1, -1]], dtype=np.int8)
    ver = dict(identity=np.array([[0.9, 0.95, 0.95, 0.95, 0.0]]), aln_cols=np.array([[100, 100, 100, 100, 0]]), n_match=np.array([[90, 95, 95, 95, 0]]),
               q_cov=np.array([[0.8, 0.8, np.nextafter(0.8, 0), 1.0, 0.0]]), r_cov=np.array([[1.0, 1.0, 1.0, 1.0, 0.0]]))
    ver["identity"][0, 3] = 0.95; cand_shared[0, 3] = 31
    hits = classify.rank(cand_ref, cand_shared, cand_strand, ver, min_identity=0.9, min_query_cov=0.8)[0]
    assert [h["ref"] for h in hits] == [5, 3, 9, 7]                     # identity, then shared, then the smaller reference; the -1 slot is gone
    assert [h["called"] for h in hits] == [True, True, False, True]      # q_cov just below 0.8 is not called; identity == 0.9 and q_cov == 0.8 are
    hits = classify.rank(cand_ref, cand_shared, cand_strand, ver, min_identity=np.nextafter(0.9, 1), min_query_cov=0.8)[0]
    assert [h["called"] for h in hits] == [True, True, False, False]
    assert classify.rank(np.full((2, 3), -1), np.full((2, 3), -1), np.full((2, 3), -1), {k: np.zeros((2, 3)) for k in ver}) == [[], []]


def test_read_reference_fasta(tmp_path):
    p = tmp_path / "lib.fasta"
    p.write_text(">sp1 Genus species|COI-5P\nACGTAC\nGTACGT\n\n>sp2\tother words\nacgtRYKM\nNNAC\n>sp3\nAC-GT\n")
    lib = classify.read_reference_fasta(str(p))
    assert lib.names == ["sp1", "sp2", "sp3"] and lib.headers == ["sp1 Genus species|COI-5P", "sp2\tother words", "sp3"]
    assert [lib.rs.get(i)[0] for i in range(3)] == ["ACGTACGTACGT", "ACGTNNNNNNAC", "ACNGT"] and lib.changed == 9 and len(lib) == 3
    p.write_text(">a\nACGT\n>b\nAC\n>a desc\nGG\n")
    with pytest.raises(ValueError, match="record 3.*record 1"):
        classify.read_reference_fasta(str(p))
    assert classify.read_reference_fasta(str(p), unique_names=False).names == ["a", "b", "a"]
    p.write_text(">a\nACGT\n>b\n\n>c\nAC\n")
    with pytest.raises(ValueError, match="record 2"):
        classify.read_reference_fasta(str(p))
    p.write_text(">a\nACGT\n>b\n")
    with pytest.raises(ValueError, match="record 2"):
        classify.read_reference_fasta(str(p))


def test_table_text(tmp_path):
    lib = classify.Library(["sp1", "sp2"], ["sp1 Genus one", "sp2"], None, 0)
    hits = [[dict(ref=1, strand=1, shared=41, identity=0.1 + 0.2, aln_cols=650, n_match=195, q_cov=1.0, r_cov=2 / 3, called=False),
             dict(ref=0, strand=0, shared=7, identity=1e-05, aln_cols=3, n_match=0, q_cov=0.5, r_cov=1e22, called=True)], []]
    rows = classify.table_rows(["consensus_cl_id_4_total_supporting_reads_120", "other"], [120, 0], hits, lib, report=5)
    classify.write_table(str(tmp_path / "t.tsv"), rows)
    assert (tmp_path / "t.tsv").read_text() == (
        "#consensus_id\tn_reads\trank\treference\tstrand\tshared\tidentity\taln_cols\tn_match\tq_cov\tr_cov\tcalled\theader\n"
        "consensus_cl_id_4_total_supporting_reads_120\t120\t1\tsp2\t-\t41\t0.30000000000000004\t650\t195\t1.0\t0.6666666666666666\t0\tsp2\n"
        "consensus_cl_id_4_total_supporting_reads_120\t120\t2\tsp1\t+\t7\t1e-05\t3\t0\t0.5\t1e+22\t1\tsp1 Genus one\n"
        "other\t0\t0\t*\t*\t0\t0.0\t0\t0\t0.0\t0.0\t0\t*\n")
    one = classify.table_rows(["x"], [3], hits[:1], lib, report=1, sample="s1")
    classify.write_table(str(tmp_path / "all.tsv"), one, with_sample=True)
    assert (tmp_path / "all.tsv").read_text().splitlines()[1].split("\t")[:4] == ["s1", "x", "3", "1"] and len(one) == 1
    assert classify.n_reads_of("consensus_cl_id_4_total_supporting_reads_120") == 120 and classify.n_reads_of("abc") == 0


@pytest.mark.parametrize("flags", [["--reference_db", "LIB"], ["--consensus", "--reference_db", "LIB", "--classify_k", "22"],
                                   ["--consensus", "--reference_db", "LIB", "--classify_top_k", "65"], ["--consensus", "--reference_db", "LIB", "--classify_top_k", "0"],
                                   ["--consensus", "--reference_db", "LIB", "--classify_w", "12"], ["--consensus", "--reference_db", "missing.fasta"]])
def test_cli_refuses(tmp_path, flags):
    from ngspeciesid_amd.cli import cli
    lib = tmp_path / "lib.fasta"; lib.write_text(">a\nACGT\n")
    fq = tmp_path / "r.fastq"; fq.write_text("@r\nACGT\n+\nIIII\n")
    flags = [str(lib) if f == "LIB" else f for f in flags]
    with pytest.raises(SystemExit) as e:
        cli(["--ont", "--fastq", str(fq), "--outfolder", str(tmp_path / "o"), "--t", "1"] + flags)
    assert e.value.code == 1 and not (tmp_path / "o").exists()
    with pytest.raises(SystemExit) as e:                                             # the sub-command checks the same ranges
        cli(["classify", "--fasta", str(lib), "--reference_db", str(lib), "--outfile", str(tmp_path / "t.tsv"), "--classify_k", "22"])
    assert e.value.code == 1 and not (tmp_path / "t.tsv").exists()
