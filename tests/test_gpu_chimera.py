"""GPU: ngsid_chimera_model (include/ngsid_chimera.h, csrc/k_chimera.hip) through Api.chimera_model against tests/chimera_reference.py.  Every comparison is exact
equality of the seven fields AND of the profiles.  The last tests run the policy layer (chimera.py) on reads of three species and one constructed chimera, through
pipeline.run_hot_path and through the command line."""
import os
import numpy as np
import pytest
import chimera_reference as ref
import chimera_cases as cases
from ngspeciesid_amd import runtime, classify
from ngspeciesid_amd._capi import ReadSet, NgsidError, CHIMERA_ROWS as R, CHIMERA_STRIP as STRIP, CHIMERA_NFIELD, CHIMERA_FIELDS, MAX_CONSENSUS_LEN

pytestmark = pytest.mark.gpu
BORDERS = (0, 1, 2, R - 1, R, R + 1, 63, 64, 65, STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + 1)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("fields", "profiles", "prof_off")):
        assert g.shape == w.shape and g.dtype == w.dtype, "%s: %s is %s %s, want %s %s" % (what, name, g.shape, g.dtype, w.shape, w.dtype)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s: %s differs at %s: got %s, want %s (%d places)" % (what, name, bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])], len(bad))


def _check(api, queries, parents, pair_off, pair_parent, pair_gid=None, what="", cache=None):
    want = ref.chimera_model(queries, parents, pair_off, pair_parent, pair_gid, cache=cache)
    got = api.chimera_model(queries, parents, pair_off, pair_parent, pair_gid, profiles=True)
    _same(got, want, what)
    plain = api.chimera_model(queries, parents, pair_off, pair_parent, pair_gid)
    assert np.array_equal(plain, want[0]), what + ": fields without profiles"
    return got


def test_constants_are_the_headers():
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "ngsid_chimera.h")).read()
    assert "#define NGSID_CHIMERA_ROWS   %d " % R in text and "#define NGSID_CHIMERA_NFIELD %d " % CHIMERA_NFIELD in text and STRIP == 64 * R and len(CHIMERA_FIELDS) == CHIMERA_NFIELD


@pytest.mark.parametrize("n", BORDERS)
def test_lengths_at_the_kernels_borders(gpu_api, n):
    """query length n against every parent length of BORDERS, 3 parents each: lane rows, wave, strip and two strips + 1"""
    rng = np.random.default_rng(100 + n)
    queries, parents, pair_off, pair_parent = [], [], [0], []
    for m in BORDERS:
        q, ps = cases.related(rng, n, m, 3)
        queries.append(q)
        pair_parent += list(range(len(parents), len(parents) + 3)); parents += ps; pair_off.append(len(pair_parent))
    got = _check(gpu_api, queries, parents, pair_off, pair_parent, what="n=%d" % n)
    assert (got[0][:, 1] <= n).all() and (got[0][:, 2] <= got[0][:, 1]).all() and (got[0][:, 2] >= 0).all()


def test_one_pair_of_the_largest_size(gpu_api):
    rng = np.random.default_rng(7)
    L = MAX_CONSENSUS_LEN
    q = cases.rand_seq(rng, L)
    p = cases.mutate(rng, q[:L // 2], 0.05)[:L // 2] + cases.rand_seq(rng, L)
    p = p[:L]
    assert len(q) == L and len(p) == L
    got = _check(gpu_api, [q], [p], [0, 1], [0], what="16384 x 16384")
    assert got[0][0, 2:].tolist() == [-1] * 5 and got[0][0, 1] > 1000


def test_pair_counts(gpu_api):
    """0, 1, 2, 3, 64, 65 and 300 pairs per query, queries with and without pairs mixed in one call"""
    rng = np.random.default_rng(11)
    pool = cases.family(rng, 12, 40, 0.1)
    pool = pool + pool[:5] + [cases.rand_seq(rng, 33), ""]
    queries, pair_off, pair_parent = [], [0], []
    for x, P in enumerate((0, 1, 300, 0, 2, 3, 64, 0, 65, 1, 0)):
        a, b = pool[int(rng.integers(0, 12))], pool[int(rng.integers(0, 12))]
        k = int(rng.integers(5, 35))
        queries.append(cases.mutate(rng, a[:k] + b[k:], 0.03))
        pair_parent += rng.integers(0, len(pool), P).tolist(); pair_off.append(len(pair_parent))
    cache = {}
    got = _check(gpu_api, queries, pool, pair_off, pair_parent, what="pair counts", cache=cache)
    assert (got[0][[0, 3, 7, 10]] == -1).all() and (got[0][[1, 9], 2:] == -1).all() and (got[0][[1, 9], :2] >= 0).all()
    gid = (np.asarray(pair_parent) % 3).astype(np.int32)
    _check(gpu_api, queries, pool, pair_off, pair_parent, gid, what="pair counts, three gids", cache=cache)


def test_ties(gpu_api):
    """duplicated parents on both sides of the 64-pair borders, a query equal to a parent, all-identical parents: the smaller pair index wins"""
    rng = np.random.default_rng(13)
    a, b, c = cases.family(rng, 3, 60, 0.15)
    q = a[:25] + b[25:]
    filler = cases.rand_seq(rng, 60)
    cache = {}
    for where in ((0, 1), (62, 63), (63, 64), (64, 65), (1, 129), (127, 128)):
        parents = [filler] * 130
        for x in where: parents[x] = a
        parents[5] = b; parents[70] = b
        got = _check(gpu_api, [q, a], parents, [0, 130, 260], list(range(130)) * 2, what="ties %s" % (where,), cache=cache)
        f = got[0]
        assert f[0, 2:5].tolist() == [0, where[0], 5] and f[0, 5] <= 25 <= f[0, 6]
        assert f[1, :2].tolist() == [where[0], 0] and f[1, 2] == 0                      # the query equals a parent
    same = _check(gpu_api, [q, a, ""], [a] * 70, [0, 70, 140, 210], [0] * 210, np.arange(210, dtype=np.int32), what="identical parents", cache=cache)[0]
    assert same[1].tolist() == [0, 0, 0, 0, 1, 0, len(a)] and same[0, 3:5].tolist() == [0, 1]
    assert same[2].tolist() == [0, 0, 0, 0, 1, 0, 0]                                  # the empty query: i = 0 only


def test_gids(gpu_api):
    rng = np.random.default_rng(17)
    x, y, z = cases.family(rng, 3, 80, 0.12)
    x1 = x[:60] + ("A" if x[60] != "A" else "C") + x[61:]                           # one edit away from x, behind the crossover
    q = x[:40] + y[40:]
    parents = [x, x1, y, z]
    both = classify.both_strands(ReadSet.from_strings(parents))
    strands = [both.get(i)[0] for i in range(both.n)]
    cache = {}
    # pair_gid NULL: the gid is the parent index
    f = _check(gpu_api, [q], parents, [0, 4], [0, 1, 2, 3], None, "no gids", cache)[0]
    assert f[0, 2:5].tolist() == [0, 0, 2] and f[0, 5] <= 40 <= f[0, 6]
    # best and second-best F (x, x1) in one gid; best B (y) in the same gid: the answer needs the best pair of ANOTHER gid on one side
    f = _check(gpu_api, [q], parents, [0, 4], [0, 1, 2, 3], [5, 5, 5, 9], "two best in one gid", cache)[0]
    assert f[0, 2] > 0 and 3 in f[0, 3:5].tolist()
    f = _check(gpu_api, [q], parents, [0, 4], [0, 1, 2, 3], [5, 5, 9, 5], "y alone in its gid", cache)[0]
    assert f[0, 2:5].tolist() == [0, 0, 2] and f[0, 5] <= 40 <= f[0, 6]
    # both strands of every parent as two pairs of one gid
    gid = np.repeat(np.arange(4, dtype=np.int32), 2)
    f = _check(gpu_api, [q, classify.both_strands(ReadSet.from_strings([q])).get(1)[0]], strands, [0, 8, 16], list(range(8)) * 2, np.tile(gid, 2), "both strands", cache)[0]
    assert f[0, 2:5].tolist() == [0, 0, 4] and f[1, 2:5].tolist() == [0, 5, 1] and f[0, 5] <= 40 <= f[0, 6] and f[1, 5] <= len(q) - 40 <= f[1, 6]
    # all gids equal: no two-parent model
    f = _check(gpu_api, [q], parents, [0, 4], [0, 1, 2, 3], [2, 2, 2, 2], "one gid", cache)[0]
    assert f[0, 2:].tolist() == [-1] * 5 and f[0, 0] >= 0


def test_random_small_cases_with_ties_and_gids(gpu_api):
    """400 queries of 0 .. 12 letters over two- and four-letter alphabets, up to 6 pairs, gids from {0, 1, 2}: ties everywhere"""
    rng = np.random.default_rng(19)
    queries, parents, pair_off, pair_parent, gid = cases.random_small(rng, 400)
    _check(gpu_api, queries, parents, pair_off, pair_parent, gid, "random small")


def test_n_in_queries_and_parents(gpu_api):
    rng = np.random.default_rng(23)
    a, b = cases.family(rng, 2, 90, 0.1)
    an = a[:10] + "N" + a[11:50] + "NNN" + a[53:]
    q = an[:45] + b[45:70] + "N" + b[71:]
    got = _check(gpu_api, [q, "N" * 20, an], [a, an, b, "N" * 30, ""], [0, 5, 10, 15], list(range(5)) * 3, what="N")[0]
    assert got[1, :2].tolist() == [3, 0] and got[2, :2].tolist() == [1, 0]


def test_chunking_and_residence():
    rng = np.random.default_rng(29)
    pool = cases.family(rng, 9, 150, 0.08) + [cases.rand_seq(rng, STRIP + 30)]
    queries = [cases.mutate(rng, pool[i % 9][:70] + pool[(i + 4) % 9][70:], 0.02) for i in range(10)] + ["", pool[9][:STRIP]]
    pair_off = [0]; pair_parent = []
    for i in range(len(queries)):
        pair_parent += rng.permutation(10)[:(i * 3) % 11].tolist(); pair_off.append(len(pair_parent))
    want = ref.chimera_model(queries, pool, pair_off, pair_parent)
    with runtime.new_api() as api:
        _same(api.chimera_model(queries, pool, pair_off, pair_parent, profiles=True), want, "default chunk")
        for val in (1, 3):
            api.set_option("chimera_chunk_queries", val)
            _same(api.chimera_model(queries, pool, pair_off, pair_parent, profiles=True), want, "chimera_chunk_queries=%d" % val)
        api.set_option("chimera_chunk_queries", 0)
        dq, dp = api.upload_reads(ReadSet.from_strings(queries)), api.upload_reads(ReadSet.from_strings(pool))
        try:
            assert np.array_equal(api.chimera_model(dq, dp, pair_off, pair_parent), want[0]), "device-resident read sets"
        finally:
            dq.release(); dp.release()
        api.set_option("release_scratch", 1)
        _same(api.chimera_model(queries, pool, pair_off, pair_parent, profiles=True), want, "after release_scratch")
        empty = api.chimera_model([], pool, [0], [], profiles=True)
        assert empty[0].shape == (0, CHIMERA_NFIELD) and len(empty[1]) == 0 and empty[2].tolist() == [0]


def test_errors_come_back_as_return_codes(gpu_api):
    a, b = "ACGTTGCATGCCGATAGGCTTAACGG", "TTGACCGGTAACGTTAGCATCGGCTA"
    for args, code in ((([a], [a, b[:5] + "c" + b[6:]], [0, 2], [0, 1]), -3),          # a lower-case letter in a parent
                       (([a[:3] + "t" + a[4:]], [a, b], [0, 2], [0, 1]), -3),          # ... in a query
                       (([a], [a, b], [0, 2], [0, 2]), -2),                            # a parent index out of range
                       (([a, b], [a, b], [0, 2, 1], [0]), -2),                         # decreasing offsets
                       (([a], [a, "ACGT" * 4096 + "A"], [0, 2], [0, 1]), -6),          # 16 385 bases
                       ((["ACGT" * 4096 + "A"], [a], [0, 1], [0]), -6)):
        with pytest.raises(NgsidError) as e:
            gpu_api.chimera_model(*args)
        assert e.value.code == code, args[2:]
    assert gpu_api.chimera_model([a], [a, b], [0, 2], [0, 1]).tolist() == [[0, 0, 0, 1, 0, 0, 0]]      # the context is usable after every refusal


# ---- end to end: three species and one constructed chimera
def _chimera_reads(n=400, seed=5):
    """reads of species 0 and 1 (40 % each), species 2 and the chimera head of 0 + tail of 1 (10 % each).  At 25 % divergence the chimera's reads form their own cluster
    and its polished consensus equals the constructed sequence (tried with the CPU oracle through pipeline.run_hot_path before the GPU saw it; the cluster also draws
    reads of its parents, which is why the parents are made four times as abundant: the abundance skew of 2 has to hold for the cluster sizes)
    -> (reads dict, the four sequences, crossover)"""
    from ngspeciesid_amd import synth
    sp = synth.make_species(3, 420, 0.25, seed=12)
    s0, s1 = sp[0].tobytes().decode(), sp[1].tobytes().decode()
    k = len(s0) // 2
    chim = s0[:k] + s1[len(s1) - (len(s0) - k):]
    species = list(sp) + [np.frombuffer(chim.encode(), dtype=np.uint8)]
    rd = synth.make_reads(species, n, mu=18.0, seed=seed, abundance=[0.4, 0.4, 0.1, 0.1])
    return rd, [s.tobytes().decode() for s in species], k


def _sorted_set(api, rd):
    from ngspeciesid_amd.hostutil import subset_reads
    rs = ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64))
    score, _, keep = api.score_reads(rs, 13, 7.0)
    idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
    return subset_reads(rs, idx), score[idx]


def _assert_the_chimera(entries, seqs, truth, k):
    called = [x for x, e in enumerate(entries) if e["chimeric"]]
    assert len(called) == 1 and seqs[called[0]] == truth[3], (called, [s in truth for s in seqs])
    e = entries[called[0]]
    assert seqs[e["parent_a"]] == truth[0] and seqs[e["parent_b"]] == truth[1] and e["strand_a"] == 0 and e["strand_b"] == 0
    assert e["model_ed"] == 0 and e["gain"] == e["best_ed"] > 20 and e["bp_lo"] <= k <= e["bp_hi"]


def test_run_hot_path_calls_exactly_the_chimera(gpu_api):
    from ngspeciesid_amd import pipeline, chimera
    from ngspeciesid_amd.ptable import select_p_table
    rd, truth, k = _chimera_reads()
    sub, score = _sorted_set(gpu_api, rd)
    kw = dict(k=13, w=20, abundance_ratio=0.05, racon_iter=2, p_shared=select_p_table(13, 20))
    rank = np.arange(sub.n, dtype=np.uint32)
    res = pipeline.run_hot_path(gpu_api, sub, score, acc_rank=rank, chimeras=True, **kw)
    plain = pipeline.run_hot_path(gpu_api, sub, score, acc_rank=rank, **kw)
    assert "chimeras" not in plain and [c[:4] for c in plain["centers"]] == [c[:4] for c in res["centers"]]
    seqs = [c[3] for c in res["centers"]]
    assert len(res["chimeras"]) == len(seqs) == 4 and res["chimeras"] == chimera.detect(gpu_api, seqs, [c[0] for c in res["centers"]])[0]
    _assert_the_chimera(res["chimeras"], seqs, truth, k)
    assert pipeline.run_hot_path(gpu_api, sub, score, do_consensus=False, chimeras=True, **kw)["chimeras"] == []
    assert all(not e["chimeric"] for e in pipeline.run_hot_path(gpu_api, sub, score, acc_rank=rank, chimeras=True, chimera_kwargs=dict(min_gain=1000), **kw)["chimeras"])
    # the same sample twice around an empty one, in one pass: per sample what the sample gives alone
    allr = ReadSet(np.concatenate([sub.seq, sub.seq]), np.concatenate([sub.qual, sub.qual]), np.concatenate(([0], np.cumsum(np.tile(np.diff(sub.off.astype(np.int64)), 2)))).astype(np.uint64))
    many = pipeline.run_hot_path_samples(gpu_api, allr, np.tile(score, 2), [0, sub.n, sub.n, 2 * sub.n], acc_rank=np.tile(rank, 2), chimeras=True, **kw)
    assert many[0]["chimeras"] == res["chimeras"] and many[2]["chimeras"] == res["chimeras"] and many[1]["chimeras"] == [] and many[1]["centers"] == []


def _files(folder):
    out = {}
    for root, _, fs in os.walk(folder):
        for f in fs:
            out[os.path.relpath(os.path.join(root, f), folder)] = open(os.path.join(root, f), "rb").read()
    return out


def _table_from_fasta(got, prefix, text, tmp_path, name):
    """the `chimeras` sub-command over the run's own consensus.fasta files, in the table's order -> its table as text"""
    from ngspeciesid_amd.cli import cli
    ids = [l.split("\t")[0] for l in text.splitlines()[1:]]
    fasta = tmp_path / (name + ".fasta")
    with open(fasta, "w") as fh:
        for i in ids:
            fh.write(got["%sracon_cl_id_%s/consensus.fasta" % (prefix, i.split("_")[3])].decode())
    with pytest.raises(SystemExit) as e:
        cli(["chimeras", "--fasta", str(fasta), "--outfile", str(tmp_path / (name + ".tsv"))])
    assert e.value.code == 0
    return open(tmp_path / (name + ".tsv")).read()


def test_cli_chimeras_equals_the_subcommand(gpu_api, tmp_path):
    from ngspeciesid_amd.cli import cli
    from ngspeciesid_amd import synth, chimera
    rd, truth, k = _chimera_reads()
    fq = str(tmp_path / "r.fastq")
    synth.reads_to_fastq(rd, fq)
    flags = ["--ont", "--fastq", fq, "--t", "1", "--consensus", "--racon", "--racon_iter", "2", "--abundance_ratio", "0.05"]
    cli(flags + ["--outfolder", str(tmp_path / "A"), "--chimeras"])
    cli(flags + ["--outfolder", str(tmp_path / "B")])
    got, plain = _files(str(tmp_path / "A")), _files(str(tmp_path / "B"))
    assert sorted(k_ for k_ in got if k_ not in plain) == ["chimeras.tsv"] and all(got[k_] == plain[k_] for k_ in plain if not k_.endswith("logfile.txt"))
    text = got["chimeras.tsv"].decode()
    assert text.splitlines()[0] == "#" + "\t".join(chimera.COLUMNS)
    assert _table_from_fasta(got, "", text, tmp_path, "one") == text
    rows = chimera.read_table(str(tmp_path / "A" / "chimeras.tsv"))
    seq_of = {r["id"]: got["racon_cl_id_%s/consensus.fasta" % r["id"].split("_")[3]].decode().split("\n")[1] for r in rows}
    called = [r for r in rows if r["chimeric"]]
    assert len(called) == 1 and seq_of[called[0]["id"]] == truth[3]
    c = called[0]
    assert seq_of[c["parent_a"]] == truth[0] and seq_of[c["parent_b"]] == truth[1] and (c["strand_a"], c["strand_b"]) == ("+", "+") and c["model_ed"] == 0 and c["bp_lo"] <= k <= c["bp_hi"]


def test_cli_fastq_dir_writes_a_table_per_sample(gpu_api, tmp_path):
    from ngspeciesid_amd.cli import cli
    from ngspeciesid_amd import synth, chimera
    d = tmp_path / "in"; d.mkdir()
    rd, truth, k = _chimera_reads()
    synth.reads_to_fastq(rd, str(d / "s_one.fastq"), prefix="a")
    sp = synth.make_species(2, 420, 0.25, seed=3)
    synth.reads_to_fastq(synth.make_reads(sp, 200, mu=18.0, seed=9), str(d / "s_two.fastq"), prefix="b")
    cli(["--ont", "--fastq_dir", str(d), "--t", "1", "--consensus", "--racon", "--racon_iter", "2", "--abundance_ratio", "0.05", "--outfolder", str(tmp_path / "A"), "--chimeras"])
    got = _files(str(tmp_path / "A"))
    assert sorted(k_ for k_ in got if "chimeras" in k_) == ["chimeras_all.tsv", "s_one/chimeras.tsv", "s_two/chimeras.tsv"]
    everything = []
    for name in ("s_one", "s_two"):
        text = got[name + "/chimeras.tsv"].decode()
        assert _table_from_fasta(got, name + "/", text, tmp_path, name) == text
        everything += [name + "\t" + l for l in text.splitlines()[1:]]
    all_text = got["chimeras_all.tsv"].decode().splitlines()
    assert all_text[0] == "#sample\t" + "\t".join(chimera.COLUMNS) and all_text[1:] == everything
    assert sum(r["chimeric"] for r in chimera.read_table(str(tmp_path / "A" / "s_one" / "chimeras.tsv"))) == 1
    assert sum(r["chimeric"] for r in chimera.read_table(str(tmp_path / "A" / "s_two" / "chimeras.tsv"))) == 0
