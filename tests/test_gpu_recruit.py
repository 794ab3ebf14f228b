"""GPU: ngsid_recruit (include/ngsid_recruit.h, csrc/k_recruit.hip) against the numpy restatement of its definition (tests/recruit_reference.py), array for array, on
the cases of tests/recruit_cases.py; chunking, device-resident reads, the error codes; the pipeline key and the command-line flag."""
import os
import numpy as np
import pytest
import recruit_cases as cases
import recruit_reference as ref
from ngspeciesid_amd import pipeline, recruit, synth
from ngspeciesid_amd._capi import NgsidError, ReadSet

pytestmark = pytest.mark.gpu


def _call(api, c, rs=None):
    return api.recruit(ReadSet.from_strings(c["reads"]) if rs is None else rs, c["read_off"], c["cons"], c["cons_off"], c["max_ed"], both_strands=c["both"])


def _same(got, want, c, what=""):
    assert got.dtype == np.int32 and got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, [(int(r), got[r].tolist(), want[r].tolist(), len(c["reads"][r])) for r in bad[:5]])


@pytest.mark.parametrize("name", cases.NAMES)
def test_cases_equal_the_reference(gpu_api, name):
    c = cases.build(name)
    want = cases.expected(name)
    _same(_call(gpu_api, c), want, c, name)
    try:                                                                # with or without the cut-off rule the outputs are identical
        for family in (1, 2):
            gpu_api.set_option("recruit_cutoff", family)
            _same(_call(gpu_api, c), want, c, "%s, %s instances" % (name, ("plain", "cut-off")[family - 1]))
    finally:
        gpu_api.set_option("recruit_cutoff", 0)
    assert (want[:, 0] >= 0).any() and (name == "pattern_lengths" or (want[:, 0] < 0).any())      # reads with and without a consensus
    if name == "pattern_lengths":                                      # every instance of the family is taken, and every group finds its planted reads on both strands
        assert {min(w for w in cases.INSTANCE_WORDS if 64 * w >= len(p)) for p in c["cons"]} == set(cases.INSTANCE_WORDS)
        assert (want[:, 0] >= 0).all() and set(want[:, 2].tolist()) == {0, 1} and (want[:, 4] >= 0).all()
    if name == "reduction_both":
        assert (want[want[:, 0] >= 0, 2] == 1).any() and (want[:, 5] == want[:, 1])[want[:, 4] >= 0].any()
    if name == "reduction_one_strand":
        assert (want[:, 2] == 0).all()
    if name == "cutoff":
        assert (want[cases.CUTOFF_PLANTED, 0] >= 0).mean() >= 0.9


def test_chunking_and_device_resident_reads(gpu_api):
    """the same call under "recruit_chunk_reads" of 1, 64, 100 and the default, on host and device-resident reads: identical arrays"""
    c = cases.build("groups")
    want = cases.expected("groups")
    rs = ReadSet.from_strings(c["reads"])
    dev = gpu_api.upload_reads(rs)
    try:
        for chunk in (1, 64, 100, 0):
            gpu_api.set_option("recruit_chunk_reads", chunk)
            _same(_call(gpu_api, c, rs), want, c, "chunks of %d, host" % chunk)
            if chunk in (100, 0): _same(_call(gpu_api, c, dev), want, c, "chunks of %d, device" % chunk)
    finally:
        gpu_api.set_option("recruit_chunk_reads", 0)
        dev.release()


def test_no_reads_and_no_groups(gpu_api):
    assert gpu_api.recruit(ReadSet.from_strings([]), [0], [], [0], []).shape == (0, 6)
    assert gpu_api.recruit(ReadSet.from_strings([]), [0, 0], ["ACGT"], [0, 1], [1]).shape == (0, 6)
    assert gpu_api.recruit(ReadSet.from_strings(["ACGT", ""]), [0, 2], [], [0, 0], []).tolist() == [list(ref.NONE)] * 2


def test_argument_errors(gpu_api):
    """each error returns its code, and hits stays as the binding filled it"""
    reads = ReadSet.from_strings(["ACGTACGT", "TTTT"])
    for args, code in (((reads, [0, 2], ["ACGT", ""], [0, 2], [1, 1]), -2),                 # an empty consensus
                       ((reads, [0, 2], ["ACGT"], [0, 1], [-1]), -2),                      # a negative max_ed
                       ((reads, [0, 2], ["A" * 2049], [0, 1], [5]), -6),                   # 2 049 letters
                       ((reads, [0, 2], ["ACgT"], [0, 1], [1]), -3),                       # a lower-case letter in a consensus
                       ((ReadSet.from_strings(["ACGT", "AcGT"]), [0, 2], ["ACGT"], [0, 1], [1]), -3),      # ... in a read
                       ((reads, [0, 2, 1, 2], ["ACGT"] * 3, [0, 1, 2, 3], [1, 1, 1]), -2),  # read offsets not monotone
                       ((reads, [0, 1, 2], ["ACGT"] * 2, [0, 2, 1], [1, 1]), -2),           # consensus offsets not monotone
                       ((reads, [0, 1], ["ACGT"], [0, 1], [1]), -2),                       # the offsets do not cover the reads
                       ((reads, [1, 2], ["ACGT"], [0, 1], [1]), -2)):
        with pytest.raises(NgsidError) as e:
            gpu_api.recruit(*args)
        assert e.value.code == code, args[1:]
    # hits is not written: the library's own entry, a buffer of a sentinel value
    import ctypes as C
    from ngspeciesid_amd._capi import _p
    cons = ReadSet.from_strings(["A" * 2049]); hits = np.full((2, 6), 77, dtype=np.int32)
    ro = np.array([0, 2], dtype=np.uint64); co = np.array([0, 1], dtype=np.uint64); me = np.array([5], dtype=np.int32)
    assert gpu_api._call("recruit", C.byref(reads.c), _p(ro), C.byref(cons.c), _p(co), C.c_uint64(1), _p(me), C.c_uint32(1), _p(hits)) == -6 and (hits == 77).all()
    assert gpu_api.recruit(reads, [0, 2], ["A" * 2048, "ACGT"], [0, 2], [5, 0]).tolist() == [[1, 0, 0, 3, -1, -1], list(ref.NONE)]      # the call after an error works


# ---- the pipeline and the command line
@pytest.fixture(scope="module")
def sample(oracle):
    """two templates of 300 bases 15 % apart, about 2 000 reads at the noisy profile on both strands, in score order as the pipeline takes them"""
    from ngspeciesid_amd.hostutil import subset_reads
    from ngspeciesid_amd.ptable import select_p_table
    sp = synth.make_species(2, 300, 0.15, seed=31)
    rd = synth.make_reads(sp, 1000, mu=14.0, seed=32, rc_fraction=0.5)
    rs = ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64))
    score, err, keep = oracle.score_reads(rs, 13, 7.0)
    idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
    sub = subset_reads(rs, idx)
    return rs, sub, score[idx], dict(k=13, w=20, abundance_ratio=0.05, racon_iter=2, band=0, p_shared=select_p_table(13, 20), acc_rank=np.arange(sub.n, dtype=np.uint32))


def _check_sample(res, plain, reads):
    assert sorted(plain) == sorted(k for k in res if k != "recruit") and sorted(res["recruit"]) == ["counts", "hits", "status"]
    for k in plain:
        if k == "centers": assert res[k] == plain[k]
        elif isinstance(plain[k], np.ndarray): assert np.array_equal(res[k], plain[k])
    finals = [c[3] for c in res["centers"]]
    want = ref.recruit(reads, [0, len(reads)], finals, [0, len(finals)], recruit.thresholds([len(q) for q in finals]))
    got = res["recruit"]
    assert np.array_equal(got["hits"], want) and np.array_equal(got["status"], recruit.assign(want))
    assert len(got["counts"]["centres"]) == len(finals) >= 2
    # every centre recruits at least those of its own pooled reads that the reference assigns to it
    rep = res["rep_of"]
    st = recruit.assign(want)
    for i, (c, cnt) in enumerate(zip(res["centers"], got["counts"]["centres"])):
        own = np.isin(rep, c[4])
        mine = int((own & (want[:, 0] == i) & (st == recruit.ASSIGNED)).sum())
        assert cnt["reads_clustered"] == c[0] and cnt["reads_recruited"] >= mine > 0 and cnt["from_own_clusters"] == mine
        assert cnt["reads_recruited"] == cnt["from_own_clusters"] + cnt["from_other_centres"] + cnt["from_unclustered"]
    assert sum(cnt["reads_recruited"] for cnt in got["counts"]["centres"]) + got["counts"]["ambiguous"] + got["counts"]["unassigned"] == len(reads)
    return want


def test_pipeline_key(gpu_api, sample):
    _, sub, score, kw = sample
    reads = [sub.get(i)[0] for i in range(sub.n)]
    T = {}
    res = pipeline.run_hot_path(gpu_api, sub, score, recruit=True, timings=T, **kw)
    plain = pipeline.run_hot_path(gpu_api, sub, score, **kw)
    want = _check_sample(res, plain, reads)
    assert T["recruit"] > 0 and (want[:, 0] >= 0).mean() > 0.5          # the comparison is not one of -1 against -1
    # without consensus stages: every read unassigned
    none = pipeline.run_hot_path(gpu_api, sub, score, recruit=True, do_consensus=False, **kw)
    assert none["recruit"]["counts"] == dict(centres=[], ambiguous=0, unassigned=sub.n) and none["recruit"]["hits"].tolist() == [list(ref.NONE)] * sub.n
    # one-strand mode and a margin through recruit_kwargs
    one = pipeline.run_hot_path(gpu_api, sub, score, recruit=True, recruit_kwargs=dict(both_strands=False, min_margin=3, min_identity=0.85), **kw)
    finals = [c[3] for c in one["centers"]]
    w1 = ref.recruit(reads[:300], [0, 300], finals, [0, len(finals)], recruit.thresholds([len(q) for q in finals], 0.85), both_strands=False)
    assert np.array_equal(one["recruit"]["hits"][:300], w1) and np.array_equal(one["recruit"]["status"][:300], recruit.assign(w1, 3)) and (one["recruit"]["hits"][:, 2] == 0).all()


def test_pipeline_samples(gpu_api, sample):
    """run_hot_path_samples on two samples (and an empty one between them) equals the per-sample runs"""
    from ngspeciesid_amd.hostutil import subset_reads
    _, sub, score, kw = sample
    kw = {k: v for k, v in kw.items() if k != "acc_rank"}
    n2 = sub.n // 2
    second = subset_reads(sub, np.arange(0, n2))
    both = ReadSet(np.concatenate([sub.seq, second.seq]), np.concatenate([sub.qual, second.qual]), np.concatenate([sub.off, second.off[1:] + sub.off[-1]]))
    sc = np.concatenate([score, score[:n2]])
    rank = np.concatenate([np.arange(sub.n), np.arange(n2)]).astype(np.uint32)
    out = pipeline.run_hot_path_samples(gpu_api, both, sc, [0, sub.n, sub.n, sub.n + n2], recruit=True, acc_rank=rank, **kw)
    assert len(out) == 3 and out[1]["recruit"]["hits"].shape == (0, 6) and out[1]["recruit"]["counts"] == dict(centres=[], ambiguous=0, unassigned=0)
    for o, (rs_, s_) in zip((out[0], out[2]), ((sub, score), (second, score[:n2]))):
        alone = pipeline.run_hot_path(gpu_api, rs_, s_, recruit=True, acc_rank=np.arange(rs_.n, dtype=np.uint32), **kw)
        assert o["centers"] == alone["centers"] and o["recruit"]["counts"] == alone["recruit"]["counts"]
        assert np.array_equal(o["recruit"]["hits"], alone["recruit"]["hits"]) and np.array_equal(o["recruit"]["status"], alone["recruit"]["status"])


def _files(out):
    res = {}
    for root, _, fs in os.walk(out):
        for f in fs:
            res[os.path.relpath(os.path.join(root, f), out)] = open(os.path.join(root, f), "rb").read()
    return res


def test_cli_flag_under_fastq_dir(gpu_api, tmp_path, sample):
    """--fastq_dir: recount.tsv and read_assignments.tsv per sample folder - the files a run of that sample alone writes - and recount_all.tsv with the sample in front"""
    from ngspeciesid_amd import cli as _cli, fastpath
    rs = sample[0]
    os.makedirs(str(tmp_path / "in"))
    for name, n in (("s1", 400), ("s2", 300)):
        with open(str(tmp_path / "in" / (name + ".fastq")), "w") as f:
            for i in range(n):
                s, q = rs.get(i)
                f.write("@r%d\n%s\n+\n%s\n" % (i, s, q))
    common = ["--ont", "--t", "1", "--consensus", "--racon", "--racon_iter", "2", "--abundance_ratio", "0.05", "--recruit", "--recruit_min_margin", "2"]
    outs = {}
    for key, src in (("dir", ["--fastq_dir", str(tmp_path / "in")]), ("s1", ["--fastq", str(tmp_path / "in" / "s1.fastq")]), ("s2", ["--fastq", str(tmp_path / "in" / "s2.fastq")])):
        out = str(tmp_path / ("o_" + key)); os.makedirs(out)
        args = _cli.build_parser().parse_args(src + ["--outfolder", out] + common); args.k, args.w = 13, 20
        fastpath.main(args, api=gpu_api)
        outs[key] = _files(out)
    want = ["\t".join(["sample", "consensus"] + list(recruit.RECOUNT_COLUMNS))]
    for s in ("s1", "s2"):
        for f in ("recount.tsv", "read_assignments.tsv"):
            assert outs["dir"][os.path.join(s, f)] == outs[s][f] and len(outs[s][f].decode().splitlines()) > 3
        lines = outs[s]["recount.tsv"].decode().splitlines()
        want += [s + "\t" + l for l in lines[1:-2]] + ["%s\t%s\t%s" % (l.split("\t")[0], s, l.split("\t")[1]) for l in lines[-2:]]
    assert outs["dir"]["recount_all.tsv"].decode().splitlines() == want
    assert sorted(f for f in outs["dir"] if os.sep not in f) == ["recount_all.tsv"]


def test_cli_flag_and_sub_command(gpu_api, tmp_path, sample):
    """--consensus --racon --recruit: the two new files parse, every other output file is byte-identical to the run without the flag; the `recruit` sub-command on the
    run's own reads and consensuses gives the same assignments"""
    from ngspeciesid_amd import cli as _cli, fastpath
    rs = sample[0]
    fq = str(tmp_path / "in.fastq")
    n = 400
    with open(fq, "w") as f:
        for i in range(n):
            s, q = rs.get(i)
            f.write("@r%d\n%s\n+\n%s\n" % (i, s, q))
    res = []
    for flag in ([], ["--recruit"]):
        out = str(tmp_path / ("o%d" % len(flag))); os.makedirs(out)
        args = _cli.build_parser().parse_args(["--ont", "--fastq", fq, "--outfolder", out, "--t", "1", "--consensus", "--racon", "--racon_iter", "2", "--abundance_ratio", "0.05"] + flag); args.k, args.w = 13, 20
        r = fastpath.main(args, api=gpu_api)
        res.append(_files(out))
    a, b = res
    assert sorted(set(b) - set(a)) == ["read_assignments.tsv", "recount.tsv"] and all(a[f] == b[f] for f in a) and r["timings"]["recruit"] > 0
    rows = [l.split("\t") for l in b["recount.tsv"].decode().splitlines()]
    assert rows[0] == ["consensus"] + list(recruit.RECOUNT_COLUMNS) and [x[0] for x in rows[-2:]] == ["#ambiguous", "#unassigned"]
    centres = rows[1:-2]
    assert len(centres) == len(r["centers"]) >= 2 and [x[0] for x in centres] == [str(m[1]) for m in r["centers"]] and [int(x[1]) for x in centres] == [m[0] for m in r["centers"]]
    assert all(int(x[2]) == int(x[3]) + int(x[4]) + int(x[5]) for x in centres)
    asg = [l.split("\t") for l in b["read_assignments.tsv"].decode().splitlines()]
    n_sorted = len(b["sorted.fastq"].decode().splitlines()) // 4
    assert asg[0] == ["read", "consensus", "strand", "ed", "identity", "status"] and len(asg) == n_sorted + 1
    assert sum(int(x[2]) for x in centres) + int(rows[-2][1]) + int(rows[-1][1]) == n_sorted
    for cid, cnt in ((x[0], int(x[2])) for x in centres):
        assert sum(1 for x in asg[1:] if x[1] == cid and x[5] == "assigned") == cnt
    assert all(x[2] in "+-" and 0.8 <= float(x[4]) <= 1.0 for x in asg[1:] if x[1] != "-") and {x[5] for x in asg[1:]} <= set(recruit.STATUS_NAMES)
    # the sub-command: the sorted reads against the consensuses the run wrote
    fa = str(tmp_path / "cons.fasta")
    with open(fa, "w") as f:
        for m in r["centers"]:
            f.write(b[os.path.join("racon_cl_id_%d" % m[1], "consensus.fasta")].decode())
    args = _cli._recruit_subparser(__import__("argparse").ArgumentParser()).parse_args(["--fastq", os.path.join(str(tmp_path), "o1", "sorted.fastq"), "--fasta", fa, "--outfolder", str(tmp_path / "sub")])
    sub = recruit.recruit_fastq(args, api=gpu_api)
    asg2 = [l.split("\t") for l in open(str(tmp_path / "sub" / "read_assignments.tsv")).read().splitlines()]
    assert [x[2:] for x in asg2] == [x[2:] for x in asg] and [c["reads_recruited"] for c in sub["counts"]["centres"]] == [int(x[2]) for x in centres]
    assert [c["reads_clustered"] for c in sub["counts"]["centres"]] == [m[0] for m in r["centers"]]
    # --recruit needs --consensus
    with pytest.raises(SystemExit) as e:
        _cli.cli(["--ont", "--fastq", fq, "--outfolder", str(tmp_path / "x"), "--recruit"])
    assert e.value.code not in (0, None)
