"""GPU: ngsid_refdb_build / ngsid_classify_search (include/ngsid_classify.h, csrc/k_classify.hip) through Api.refdb_build / Api.classify_search against
tests/classify_reference.py over the library's own minimizer call.  Every comparison is exact equality of cand_ref, cand_shared, cand_strand and n_codes.  The last
tests run the policy layer (classify.py) on a library with known truth and `--reference_db` of the command line against the `classify` sub-command."""
import os
import numpy as np
import pytest
import classify_reference as ref
from ngspeciesid_amd import runtime, classify, synth
from ngspeciesid_amd._capi import ReadSet, NgsidError

pytestmark = pytest.mark.gpu
NAMES = ("cand_ref", "cand_shared", "cand_strand", "n_codes")


def _same(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        assert g.shape == w.shape and g.dtype == w.dtype, "%s: %s is %s %s, want %s %s" % (what, name, g.shape, g.dtype, w.shape, w.dtype)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s: %s differs at %s: got %s, want %s" % (what, name, bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


class Case:
    """one library and one query set: the shared counts of the reference are computed once, every (top_k, min_shared) is a numpy selection from them"""

    def __init__(self, api, refs, queries, k=13, w=20):
        self.api, self.refs, self.queries, self.k, self.w = api, list(refs), list(queries), k, w
        f, r = ref.code_sets(api, self.queries, k, w), ref.code_sets(api, [ref.revcomp(q) for q in self.queries], k, w)
        self.ncodes = np.array([[len(a), len(b)] for a, b in zip(f, r)], dtype=np.int32).reshape(len(self.queries), 2)
        self.shared = ref.shared_counts(ref.code_sets(api, self.refs, k, w), f, r)
        self.qs = ReadSet.from_strings(self.queries)

    def want(self, top_k, min_shared):
        return ref.select(self.shared, top_k, min_shared) + (self.ncodes,)

    def check(self, db, top_k, min_shared, what="", api=None, qs=None):
        got = (api or self.api).classify_search(db, self.qs if qs is None else qs, top_k=top_k, min_shared=min_shared, n_codes=True)
        _same(got, self.want(top_k, min_shared), "%s top_k=%d min_shared=%d" % (what, top_k, min_shared))
        return got


def _family_library(rng, n, lo=60, hi=400):
    """n references of lo..hi bases cut from mutated copies of a few roots: related references, so that counts tie and posting lists have more than one entry"""
    roots = [ref.rand_seq(rng, hi) for _ in range(1 + n // 16)]
    out = []
    for _ in range(n):
        s = ref.mutate(rng, roots[int(rng.integers(0, len(roots)))], 0.08)
        L = int(rng.integers(lo, hi + 1)); a = int(rng.integers(0, max(len(s) - L, 0) + 1))
        out.append(s[a:a + L])
    return out


def _queries_of(rng, refs, n):
    out = []
    for i in range(n):
        q = ref.mutate(rng, refs[int(rng.integers(0, len(refs)))], 0.03)
        if i % 3 == 2: q = ref.revcomp(q)
        if i % 10 == 9: q = ref.rand_seq(rng, 200)
        out.append(q)
    return out


@pytest.mark.parametrize("n_refs", [1, 63, 64, 65, 1025, 4097])
def test_edges_of_the_selection(gpu_api, n_refs):
    rng = np.random.default_rng(500 + n_refs)
    refs = _family_library(rng, n_refs)
    case = Case(gpu_api, refs, _queries_of(rng, refs, 40))
    with gpu_api.refdb_build(refs) as db:
        info = db.info()
        assert info["n_refs"] == n_refs and info["n_postings"] >= info["n_codes"] > 0 and info["device_bytes"] >= 4 * info["n_postings"] + 12 * info["n_codes"]
        for top_k in (1, 5, 64):                                                    # 64 is above the library size for the small libraries, 5 for the library of one
            for min_shared in (1, 3, 100000):
                got = case.check(db, top_k, min_shared, "n_refs=%d" % n_refs)
                if min_shared == 100000: assert (got[0] == -1).all() and (got[1] == -1).all() and (got[2] == -1).all()


def test_threshold_ties_take_the_smallest_indices(gpu_api):
    """100 identical copies of one reference spread over a library of 4 097, and copies on both sides of the borders between the reference ranges of the select kernel's
    four waves (ceil(n / 4) rounded up to a multiple of 64) and of its 64-lane steps"""
    n = 4097
    rng = np.random.default_rng(600)
    base = _family_library(rng, n)
    twin = ref.rand_seq(rng, 300); q = [twin, ref.revcomp(twin), ref.mutate(rng, twin, 0.02)]
    seg = ((n + 3) // 4 + 63) // 64 * 64
    assert seg == 1088
    spread = np.unique(np.linspace(3, n - 1, 100).astype(int))
    border = np.array([seg - 2, seg - 1, seg, seg + 1, 2 * seg - 1, 2 * seg, 3 * seg - 1, 3 * seg, 3 * seg + 63, 3 * seg + 64, n - 1])
    for name, where in (("spread", spread), ("borders", border), ("last wave only", np.arange(3 * seg + 100, 3 * seg + 120))):
        refs = list(base)
        for i in where: refs[int(i)] = twin
        case = Case(gpu_api, refs, q)
        with gpu_api.refdb_build(refs) as db:
            for top_k in (1, 8, 11, 64):
                got = case.check(db, top_k, 3, name)
                m = min(top_k, len(where))
                assert got[0][0, :m].tolist() == where[:m].tolist() and got[0][1, :m].tolist() == where[:m].tolist()
                assert (got[2][0, :m] == 0).all() and (got[2][1, :m] == 1).all() and (got[1][0, :m] == case.ncodes[0, 0]).all()


def test_strands(gpu_api):
    rng = np.random.default_rng(700)
    refs = [ref.rand_seq(rng, int(rng.integers(150, 400))) for _ in range(200)]
    half = ref.rand_seq(rng, 150); pal = half + ref.revcomp(half)
    refs[17] = pal
    members = [3, 50, 120, 199]
    queries = [refs[i] for i in members] + [ref.revcomp(refs[i]) for i in members] + [pal]
    case = Case(gpu_api, refs, queries)
    with gpu_api.refdb_build(refs) as db:
        got = case.check(db, 4, 3, "strands")
    for x, i in enumerate(members):
        assert got[0][x, 0] == i and got[2][x, 0] == 0 and got[0][4 + x, 0] == i and got[2][4 + x, 0] == 1 and got[1][x, 0] == got[1][4 + x, 0] > 10
        assert got[3][x].tolist() == got[3][4 + x][::-1].tolist()
    assert ref.revcomp(pal) == pal and got[0][8, 0] == 17 and got[2][8, 0] == 0 and got[3][8, 0] == got[3][8, 1]


def test_degenerate_sequences(gpu_api):
    k, w = 13, 20
    rng = np.random.default_rng(800)
    body = ref.rand_seq(rng, 300)
    odd = ["", "ACGTACGTACGT", "ACGTACGTACGTA", "A" * 500, "AC" * 300, "N" * 40, body[:100] + "NNN" + body[100:], "ACGTACGTACGTAAAAAAAA", "ACGTACGTACGT" + "N" + body[:50], body[:k], body[:w - 1]]
    refs = odd + [body, ref.revcomp(body), body[50:250]] + [ref.rand_seq(rng, 200) for _ in range(20)] + ["AC" * 300, ""]
    queries = odd + [body, ref.mutate(rng, body, 0.03), body[20:200] + "N" * 5 + body[205:], "CA" * 200, "GT" * 300]
    case = Case(gpu_api, refs, queries, k, w)
    assert case.ncodes[0].tolist() == [0, 0] and case.ncodes[1].tolist() == [0, 0] and case.ncodes[3].tolist() == [0, 0] and case.ncodes[4, 0] >= 1
    with gpu_api.refdb_build(refs, k=k, w=w) as db:
        for top_k, min_shared in ((64, 1), (3, 1), (5, 2)):
            case.check(db, top_k, min_shared, "degenerate")
    only_short = ["", "ACGT", "A" * 300]                                            # a library without any minimizer
    with gpu_api.refdb_build(only_short) as db:
        assert db.info() == dict(n_refs=3, n_postings=0, n_codes=0, device_bytes=db.info()["device_bytes"])
        Case(gpu_api, only_short, queries).check(db, 4, 1, "no postings")
        empty = gpu_api.classify_search(db, ReadSet.from_strings([]), top_k=4, n_codes=True)
        assert [a.shape for a in empty] == [(0, 4), (0, 4), (0, 4), (0, 2)]


def test_long_posting_lists(gpu_api):
    """5 000 references that all hold one 80-base stretch between unique flanks: its codes hit every reference"""
    rng = np.random.default_rng(900)
    stretch = ref.rand_seq(rng, 80)
    flanks = [(ref.rand_seq(rng, 60), ref.rand_seq(rng, 60)) for _ in range(5000)]
    refs = [a + stretch + b for a, b in flanks]
    queries = [stretch, ref.revcomp(stretch)] + [refs[i] for i in (0, 2500, 4999)] + [flanks[77][0] + stretch, ref.revcomp(stretch + flanks[4000][1]), stretch[:40]]
    case = Case(gpu_api, refs, queries)
    with gpu_api.refdb_build(refs) as db:
        for top_k, min_shared in ((5, 1), (64, 3), (1, 1)):
            got = case.check(db, top_k, min_shared, "long lists")
        got = case.check(db, 64, 1, "long lists")
    assert got[0][0].tolist() == list(range(64)) and (got[2][0] == 0).all() and (got[2][1] == 1).all()           # every reference ties: the first 64
    assert got[0][2, 0] == 0 and got[0][3, 0] == 2500 and got[0][4, 0] == 4999 and got[0][5, 0] == 77 and got[0][6, 0] == 4000 and got[2][6, 0] == 1


def test_chunking_and_residence():
    rng = np.random.default_rng(1000)
    refs = _family_library(rng, 700)
    queries = _queries_of(rng, refs, 50)
    with runtime.new_api() as api:
        case = Case(api, refs, queries)
        with api.refdb_build(refs) as db:
            plain = case.check(db, 8, 3, "default chunk")
            for name, val in (("classify_chunk_queries", 1), ("classify_chunk_queries", 3)):
                api.set_option(name, val)
                _same(api.classify_search(db, case.qs, top_k=8, min_shared=3, n_codes=True), plain, "%s=%d" % (name, val))
                api.set_option(name, 0)
            dev = api.upload_reads(case.qs)
            try:
                _same(api.classify_search(db, dev, top_k=8, min_shared=3, n_codes=True), plain, "device-resident queries")
                api.set_option("classify_chunk_queries", 7)
                _same(api.classify_search(db, dev, top_k=8, min_shared=3, n_codes=True), plain, "device-resident queries, chunks of 7")
            finally:
                dev.release()
            api.set_option("release_scratch", 1)
            _same(api.classify_search(db, case.qs, top_k=8, min_shared=3, n_codes=True), plain, "after release_scratch")


def test_two_libraries_in_one_context(gpu_api):
    rng = np.random.default_rng(1100)
    refs_a, refs_b = _family_library(rng, 300), _family_library(rng, 90)
    queries = _queries_of(rng, refs_a, 12) + _queries_of(rng, refs_b, 12)
    a, b = Case(gpu_api, refs_a, queries), Case(gpu_api, refs_b, queries)
    db_a, db_b = gpu_api.refdb_build(refs_a), gpu_api.refdb_build(refs_b)
    try:
        a.check(db_a, 8, 3, "library a")
        first = b.check(db_b, 8, 3, "library b")
        db_a.release(); db_a.release()
        _same(b.check(db_b, 8, 3, "library b after a was released"), first, "unchanged")
        with pytest.raises(NgsidError) as e:
            gpu_api.classify_search(db_a, a.qs)
        assert e.value.code == -2
    finally:
        db_a.release(); db_b.release()


@pytest.mark.parametrize("k,w", [(13, 20), (15, 50), (21, 21)])
def test_parameters(gpu_api, k, w):
    rng = np.random.default_rng(1200)
    refs = _family_library(rng, 300)
    case = Case(gpu_api, refs, _queries_of(rng, refs, 30), k, w)
    with gpu_api.refdb_build(refs, k=k, w=w) as db:
        case.check(db, 8, 3, "k=%d w=%d" % (k, w)); case.check(db, 64, 1, "k=%d w=%d" % (k, w))


def test_errors_come_back_as_return_codes(gpu_api):
    refs = ["ACGTTGCATGCCGATAGGCTTAACGGATCCATGACTGACC", "TTGACCGGTAACGTTAGCATCGGCTAAGGCTTTACGGACT"]
    qs = ReadSet.from_strings([refs[0]])
    for kw, code in ((dict(k=22, w=30), -2), (dict(k=0, w=20), -2), (dict(k=13, w=12), -2)):
        with pytest.raises(NgsidError) as e:
            gpu_api.refdb_build(refs, **kw)
        assert e.value.code == code, kw
    for bad, code in (([], -2), ([refs[0], refs[1][:20] + "a" + refs[1][21:]], -3), ([refs[0], "ACGT" * 16384 + "A"], -6)):
        with pytest.raises(NgsidError) as e:
            gpu_api.refdb_build(bad)
        assert e.value.code == code, bad[-1:][:1]
    with gpu_api.refdb_build(refs) as db:
        for kw, code in ((dict(top_k=0), -2), (dict(top_k=65), -2), (dict(min_shared=0), -2)):
            with pytest.raises(NgsidError) as e:
                gpu_api.classify_search(db, qs, **kw)
            assert e.value.code == code, kw
        with pytest.raises(NgsidError) as e:
            gpu_api.classify_search(db, ReadSet.from_strings([refs[0], refs[1][:10] + "n" + refs[1][11:]]))
        assert e.value.code == -3
        got = gpu_api.classify_search(db, qs, top_k=2, min_shared=1)              # the context is usable after every refusal
        assert got[0].tolist() == [[0, -1]] and got[2].tolist() == [[0, -1]]


TRUTH_SEED = 31      # tests/test_classify_cpu.py runs the same seed with the oracle's minimizers and aligner: the reference search + classify.verify + classify.rank recover all 60


def test_truth_through_verify_and_rank(gpu_api):
    t = ref.make_truth(TRUTH_SEED, n_members=200, length=400, divergence=0.15, n_queries=60, rate=0.03)
    case = Case(gpu_api, t["refs"], t["queries"])
    with gpu_api.refdb_build(t["refs"]) as db:
        cand_ref, cand_shared, cand_strand, _ = case.check(db, 8, 3, "truth")
        hits = classify.rank(cand_ref, cand_shared, cand_strand, classify.verify(gpu_api, t["queries"], t["refs"], cand_ref, cand_strand))
        again = classify.identify(gpu_api, db, t["queries"])
    assert again == hits
    for q, hs in enumerate(hits):
        assert hs and hs[0]["ref"] == t["member"][q] and hs[0]["strand"] == t["strand"][q] and hs[0]["called"], (q, hs[:2])


def _sample_reads(species, members, n, seed):
    """score-ordered reads of the given library members -> (ReadSet, score)"""
    from ngspeciesid_amd.hostutil import subset_reads
    rd = synth.make_reads([species[m] for m in members], n, mu=18.0, seed=seed, rc_fraction=0.3)
    rs = ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64))
    return rs


def test_run_hot_path_and_samples_return_the_ranked_hits(gpu_api):
    from ngspeciesid_amd import pipeline
    from ngspeciesid_amd.hostutil import subset_reads
    from ngspeciesid_amd.ptable import select_p_table
    species = synth.make_species(50, 420, 0.15, seed=12)
    truth = [[4, 30], [17]]
    sets, scores = [], []
    for x, members in enumerate(truth):
        rs = _sample_reads(species, members, 160, 60 + x)
        score, _, keep = gpu_api.score_reads(rs, 13, 7.0)
        idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
        sets.append(subset_reads(rs, idx)); scores.append(score[idx])
    kw = dict(k=13, w=20, racon_iter=2, p_shared=select_p_table(13, 20))
    with gpu_api.refdb_build([s.tobytes().decode() for s in species]) as db:
        one = pipeline.run_hot_path(gpu_api, sets[0], scores[0], acc_rank=np.arange(sets[0].n, dtype=np.uint32), classify=db, **kw)
        plain = pipeline.run_hot_path(gpu_api, sets[0], scores[0], acc_rank=np.arange(sets[0].n, dtype=np.uint32), **kw)
        assert "classify" not in plain and [c[:4] for c in plain["centers"]] == [c[:4] for c in one["centers"]]
        assert len(one["classify"]) == len(one["centers"]) >= 2 and one["classify"] == classify.identify(gpu_api, db, [c[3] for c in one["centers"]])
        assert sorted({hs[0]["ref"] for hs in one["classify"]}) == truth[0] and all(hs[0]["called"] for hs in one["classify"])
        none = pipeline.run_hot_path(gpu_api, sets[0], scores[0], abundance_ratio=2.0, classify=db, **kw)           # no cluster is abundant enough: no centre
        assert none["centers"] == [] and none["classify"] == []
        assert pipeline.run_hot_path(gpu_api, sets[0], scores[0], do_consensus=False, classify=db, **kw)["classify"] == []
        # both samples + an empty one in one pass: per sample what the sample gives alone
        allr = ReadSet(np.concatenate([r.seq for r in sets]), np.concatenate([r.qual for r in sets]),
                       np.concatenate(([0], np.cumsum(np.concatenate([np.diff(r.off.astype(np.int64)) for r in sets])))).astype(np.uint64))
        seg = [0, sets[0].n, sets[0].n, sets[0].n + sets[1].n]
        rank = np.concatenate([np.arange(r.n, dtype=np.uint32) for r in sets])
        many = pipeline.run_hot_path_samples(gpu_api, allr, np.concatenate(scores), seg, acc_rank=rank, classify=db, **kw)
    assert many[0]["classify"] == one["classify"] and many[1]["classify"] == [] and many[1]["centers"] == []
    assert len(many[2]["classify"]) == len(many[2]["centers"]) >= 1 and {hs[0]["ref"] for hs in many[2]["classify"]} == {17}


# ---- the command line
def _files(folder):
    out = {}
    for root, _, fs in os.walk(folder):
        for f in fs:
            out[os.path.relpath(os.path.join(root, f), folder)] = open(os.path.join(root, f), "rb").read()
    return out


def test_cli_reference_db_equals_the_classify_subcommand(gpu_api, tmp_path):
    from ngspeciesid_amd.cli import cli
    species = synth.make_species(50, 420, 0.15, seed=12)
    lib_path = str(tmp_path / "lib.fasta")
    with open(lib_path, "w") as fh:
        for i, s in enumerate(species):
            t = s.tobytes().decode()
            fh.write(">sp%02d Genus species %d\n%s\n%s\n" % (i, i, t[:200], t[200:]))
    d = tmp_path / "in"; d.mkdir()
    truth = {"s_one": [4, 30], "s_two": [17]}
    for x, (name, members) in enumerate(truth.items()):
        rd = synth.make_reads([species[m] for m in members], 160, mu=18.0, seed=40 + x, rc_fraction=0.3)
        synth.reads_to_fastq(rd, str(d / (name + ".fastq")), prefix=name)
    flags = ["--ont", "--fastq_dir", str(d), "--t", "1", "--consensus", "--racon", "--racon_iter", "2"]
    cli(flags + ["--outfolder", str(tmp_path / "A"), "--reference_db", lib_path])
    cli(flags + ["--outfolder", str(tmp_path / "B")])
    got, plain = _files(str(tmp_path / "A")), _files(str(tmp_path / "B"))
    extra = sorted(k for k in got if k not in plain)
    assert extra == ["classification_all.tsv", "s_one/classification.tsv", "s_two/classification.tsv"] and sorted(k for k in got if k in plain) == sorted(plain)
    everything = []
    for name, members in truth.items():
        text = got[name + "/classification.tsv"].decode()
        rows = [l.split("\t") for l in text.splitlines()[1:]]
        ids = list(dict.fromkeys(r[0] for r in rows))
        assert len(ids) >= len(members)
        top = {r[0]: r for r in rows if r[2] == "1"}
        assert sorted({top[i][3] for i in ids}) == sorted("sp%02d" % m for m in members) and all(top[i][11] == "1" and top[i][12].startswith(top[i][3] + " Genus") for i in ids)
        fasta = tmp_path / (name + ".fasta")                                        # the run's own consensus.fasta files, in the table's order
        with open(fasta, "w") as fh:
            for i in ids:
                c_id = i.split("_")[3]
                fh.write(got["%s/racon_cl_id_%s/consensus.fasta" % (name, c_id)].decode())
        with pytest.raises(SystemExit) as e:
            cli(["classify", "--fasta", str(fasta), "--reference_db", lib_path, "--outfile", str(tmp_path / (name + ".tsv"))])
        assert e.value.code == 0
        assert open(tmp_path / (name + ".tsv")).read() == text
        everything += [name + "\t" + l for l in text.splitlines()[1:]]
    all_text = got["classification_all.tsv"].decode().splitlines()
    assert all_text[0] == "#sample\t" + "\t".join(classify.COLUMNS) and all_text[1:] == everything


def test_cli_single_sample_writes_one_table(gpu_api, tmp_path):
    """--fastq (no samples): classification.tsv directly in the output folder, no sample column anywhere, no classification_all.tsv; without --racon the drafts are named"""
    from ngspeciesid_amd.cli import cli
    species = synth.make_species(50, 420, 0.15, seed=12)
    lib_path = str(tmp_path / "lib.fasta")
    with open(lib_path, "w") as fh:
        for i, s in enumerate(species):
            fh.write(">sp%02d\n%s\n" % (i, s.tobytes().decode()))
    fq = str(tmp_path / "r.fastq")
    synth.reads_to_fastq(synth.make_reads([species[8], species[41]], 160, mu=18.0, seed=70, rc_fraction=0.3), fq)
    for name, extra in (("P", ["--racon", "--racon_iter", "2"]), ("D", [])):
        out = tmp_path / name
        cli(["--ont", "--fastq", fq, "--outfolder", str(out), "--t", "1", "--consensus", "--reference_db", lib_path, "--classify_report", "2"] + extra)
        got = _files(str(out))
        assert "classification.tsv" in got and "classification_all.tsv" not in got
        lines = got["classification.tsv"].decode().splitlines()
        assert lines[0] == "#" + "\t".join(classify.COLUMNS)
        rows = [l.split("\t") for l in lines[1:]]
        ids = list(dict.fromkeys(r[0] for r in rows))
        assert all(1 <= sum(r[0] == i for r in rows) <= 2 for i in ids)                  # --classify_report 2
        assert sorted({r[3] for r in rows if r[2] == "1"}) == ["sp08", "sp41"] and all(r[11] == "1" for r in rows if r[2] == "1")
        seqs = {}
        for i in ids:                                                                    # the table names the final sequence of the run: polished, or the draft
            c_id = i.split("_")[3]
            path = ("racon_cl_id_%s/consensus.fasta" % c_id) if extra else ("consensus_reference_%s.fasta" % c_id)
            seqs[i] = got[path].decode().split("\n")[1]
        with gpu_api.refdb_build([s.tobytes().decode() for s in species]) as db:
            hits = classify.identify(gpu_api, db, [seqs[i] for i in ids])
        assert [[r[3] for r in rows if r[0] == i] for i in ids] == [["sp%02d" % h["ref"] for h in hs[:2]] for hs in hits]
