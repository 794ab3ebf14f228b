"""GPU: ngsid_consensus_support (include/ngsid_support.h) through the C-ABI == the definition restated from the oracle's parts (tests/support_reference.py), exactly -
counts, n_used and strand - and the pipeline / CLI layers on top of it."""
import os, time
import numpy as np
import pytest
from oracle_lib import GOLD
from ngspeciesid_amd import synth, pipeline, fastio
from ngspeciesid_amd._capi import ReadSet
from ngspeciesid_amd.hostutil import subset_reads
from ngspeciesid_amd.ptable import select_p_table
from support_reference import support_reference, _COMP

pytestmark = pytest.mark.gpu


def _rs(rd):
    return ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64))


def _concat(sets):
    seq = np.concatenate([s.seq for s in sets]); lens = np.concatenate([np.diff(s.off.astype(np.int64)) for s in sets])
    off = np.zeros(len(lens) + 1, dtype=np.uint64); off[1:] = np.cumsum(lens)
    return ReadSet(seq, None, off)


def _same(api, oracle, centres, rs, grp_off, read_order=None, k=13, w=20, clip=False, what=""):
    t0 = time.perf_counter()
    got = api.consensus_support(ReadSet.from_strings(centres), rs, grp_off, read_order=read_order, k=k, w=w, clip=clip)
    t1 = time.perf_counter()
    exp = support_reference(oracle, centres, rs, grp_off, read_order, k, w, clip)
    print("%s: %d reads, HIP %.3f s, reference %.1f s" % (what, int(grp_off[-1]), t1 - t0, time.perf_counter() - t1))
    assert np.array_equal(got[3], exp[3]), what + ": strand"
    assert np.array_equal(got[2], exp[2]), what + ": n_used"
    assert np.array_equal(got[1], exp[1])
    bad = np.nonzero((got[0] != exp[0]).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d rows differ, first %d: HIP %s reference %s" % (what, len(bad), bad[0], got[0][bad[0]].tolist(), exp[0][bad[0]].tolist())
    assert (got[0][:, 0] >= got[0][:, 1:7].sum(axis=1)).all()
    return got


def _mutate(rng, s, n_sub=0, n_del=0, n_ins=0):
    a = list(s)
    for _ in range(n_sub):
        i = int(rng.integers(len(a))); a[i] = "ACGT"[("ACGT".index(a[i]) + 1 + int(rng.integers(3))) % 4]
    for _ in range(n_del):
        del a[int(rng.integers(len(a)))]
    for _ in range(n_ins):
        a.insert(int(rng.integers(len(a) + 1)), "ACGT"[int(rng.integers(4))])
    return "".join(a)


def _rc(s):
    return _COMP[np.frombuffer(s.encode(), dtype=np.uint8)[::-1]].tobytes().decode()


def _sample_h1(api):
    rd = fastio.read_fastq(os.path.join(GOLD, "sample_h1.fastq"))
    rs = rd[1] if isinstance(rd, tuple) else rd
    score, err, keep = api.score_reads(rs, 13, 7.0)
    idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
    return subset_reads(rs, idx), score[idx]


KW = dict(k=13, w=20, abundance_ratio=0.05, racon_iter=2, band=0, p_shared=select_p_table(13, 20))


def _lists_of(res):
    """pooled read list of every centre of a run_hot_path result: the reads of its clusters (a cluster = the reads with that representative, in index order)"""
    return [np.concatenate([np.nonzero(res["rep_of"] == r)[0] for r in c[4]]).astype(np.uint32) for c in res["centers"]]


def test_sample_h1_polished_centres(gpu_api, oracle):
    sub, score = _sample_h1(gpu_api)
    kw = dict(KW, acc_rank=np.arange(sub.n, dtype=np.uint32))
    a = pipeline.run_hot_path(gpu_api, sub, score, **kw)
    b = pipeline.run_hot_path(gpu_api, sub, score, support=True, **kw)
    assert sorted(b) == sorted(list(a) + ["support"]) and a["centers"] == b["centers"]
    for key in a:
        if key != "centers": assert np.array_equal(a[key], b[key]), key
    lists = _lists_of(b); centres = [c[3] for c in b["centers"]]
    assert centres and [len(s) for s in b["support"]] == [len(c) for c in centres]
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
    got = _same(gpu_api, oracle, centres, sub, off, np.concatenate(lists), what="sample_h1")
    assert np.array_equal(np.concatenate(b["support"]), got[0])
    assert got[0][:, 0].max() > 20


def test_five_species_mixed_strands(gpu_api, oracle):
    sp = synth.make_species(5, 750, 0.15, seed=61)
    rd = synth.make_reads(sp, 2000, mu=14.0, seed=62, rc_fraction=0.5)
    rs = _rs(rd); species = rd["species"].numpy()
    lists = [np.nonzero(species == g)[0].astype(np.uint32) for g in range(5)]
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
    got = _same(gpu_api, oracle, [s.tobytes().decode() for s in sp], rs, off, np.concatenate(lists), what="5 species x 400")
    truth = rd["strand"].numpy()[np.concatenate(lists)]; called = got[3] >= 0          # (at 14 % error a few reads share no minimizer with their centre)
    assert called.mean() > 0.95 and got[2].sum() == called.sum() and np.array_equal(got[3][called], truth[called]) and 0.3 < truth.mean() < 0.7


def test_edge_groups(gpu_api, oracle):
    rng = np.random.default_rng(5)
    c = synth.make_species(3, 300, 0.3, seed=63); cs = [x.tobytes().decode() for x in c]
    unrelated = "AG" * 120
    reads = [cs[0],                                                   # group 1: one read
             unrelated, "CT" * 100,                                   # group 2: no shared minimizer
             "GGTTGGTTAACC" + cs[2] + "TTGGAACCGGTT", cs[2][40:260], _rc(cs[2]), cs[2][:100] + "NNN" + cs[2][103:], _mutate(rng, cs[2], 6, 4, 4), cs[2][:150] + "N" + cs[2][150:]]
    got = _same(gpu_api, oracle, [cs[1], cs[0], cs[1], cs[2], cs[0]], ReadSet.from_strings(reads), np.array([0, 0, 1, 3, 9, 9], dtype=np.uint64), what="edge groups")
    assert got[2].tolist() == [0, 1, 0, 6, 0] and got[3].tolist() == [0, -1, -1, 0, 0, 1, 0, 0, 0]
    # nothing listed at all, and a read set the groups list only partly and out of order
    z = gpu_api.consensus_support(ReadSet.from_strings(cs), ReadSet.from_strings(reads), np.zeros(4, dtype=np.uint64))
    assert z[0].sum() == 0 and z[2].tolist() == [0, 0, 0] and len(z[3]) == 0
    _same(gpu_api, oracle, [cs[2], cs[0]], ReadSet.from_strings(reads), np.array([0, 3, 4], dtype=np.uint64), np.array([7, 3, 5, 0], dtype=np.uint32), what="read_order")


def _length_classes(rng):
    """centres and reads that cross every instance class of the aligner: 63 / 64 / 65 bases, 769 - 896, above 1 024 and above 4 096"""
    groups = []
    for L, lens, n in ((64, (63, 64, 65), 30), (850, tuple(range(769, 897, 9)), 45), (1150, (1030, 1100, 1150, 1200), 24), (4300, (4100, 4200, 4300, 4400), 8), (400, (250, 256, 257, 400), 40), (600, (511, 512, 513, 600), 40)):
        c = synth.make_species(1, L, 0.0, seed=70 + L)[0].tobytes().decode()
        rs = []
        for x in range(n):
            l = lens[x % len(lens)]
            r = c[:l] if l <= len(c) else c + "".join("ACGT"[int(v)] for v in rng.integers(4, size=l - len(c)))
            if x % 3: r = _mutate(rng, r, n_sub=max(1, l // 40), n_del=l // 80, n_ins=l // 80)
            while len(r) < l: r += "ACGT"[int(rng.integers(4))]
            r = r[:l]
            rs.append(_rc(r) if x % 4 == 1 else r)
        groups.append((c, rs))
    return groups


def test_length_classes_alone_and_in_a_large_batch(gpu_api, oracle):
    """every group alone (fewer than 4 096 pairs: one instance chosen by the longest read - register-resident 4 / 8 / 12 blocks, sliding windows, block groups) and all of them
    behind 17 000 short reads in ONE call (the batch is partitioned by read length: class launches, two index lists in the window instance, band retries) - 20 000 reads in this file"""
    rng = np.random.default_rng(9)
    groups = _length_classes(rng)
    for c, rs in groups:
        _same(gpu_api, oracle, [c], ReadSet.from_strings(rs), np.array([0, len(rs)], dtype=np.uint64), what="alone, centre of %d" % len(c))
    sp = synth.make_species(5, 300, 0.15, seed=64)
    rd = synth.make_reads(sp, 17000, mu=14.0, seed=65, rc_fraction=0.5)
    bulk = _rs(rd); species = rd["species"].numpy()
    allrs = _concat([bulk] + [ReadSet.from_strings(rs) for _, rs in groups])
    lists = [np.nonzero(species == g)[0].astype(np.uint32) for g in range(5)]
    base = bulk.n
    for _, rs in groups:
        lists.append(np.arange(base, base + len(rs), dtype=np.uint32)); base += len(rs)
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
    centres = [s.tobytes().decode() for s in sp] + [c for c, _ in groups]
    got = _same(gpu_api, oracle, centres, allrs, off, np.concatenate(lists), what="large batch")
    # the same call in chunks of the path matrix (a budget of 1 MB: a few hundred rows at a time) and with the unbanded instances only: same integers
    for opt, val in (("support_budget_mb", 1), ("ed_band", 0)):
        gpu_api.set_option(opt, val)
        try:
            again = gpu_api.consensus_support(ReadSet.from_strings(centres), allrs, off, read_order=np.concatenate(lists))
        finally:
            gpu_api.set_option(opt, 0 if opt == "support_budget_mb" else -1)
        assert all(np.array_equal(x, y) for x, y in zip(got, again)), opt


def test_clip_on_primer_like_overhangs(gpu_api, oracle):
    rng = np.random.default_rng(13)
    c = synth.make_species(1, 500, 0.0, seed=66)[0].tobytes().decode()
    fw, rv = "TTTCTGTTGGTGCTGATATTGC", "GCAATATCAGCACCAACAGAAA"
    reads = []
    for x in range(300):
        r = _mutate(rng, fw + c + rv, n_sub=12, n_del=6, n_ins=6)
        reads.append(_rc(r) if x % 2 else r)
    reads += [c[:14] + "A" * 30, c[100:114]]                              # no run of 15 equal columns
    rs = ReadSet.from_strings(reads); off = np.array([0, len(reads)], dtype=np.uint64)
    a = _same(gpu_api, oracle, [c], rs, off, clip=True, what="clip")
    b = _same(gpu_api, oracle, [c], rs, off, clip=False, what="no clip")
    assert a[2][0] == 300 and (a[0][:, 0] <= b[0][:, 0]).all() and a[0][:, 0].sum() < b[0][:, 0].sum()


def test_planted_variant(gpu_api, oracle):
    """a group pooled 70 / 30 from two centres that differ at one base: that base has the lowest agree / depth of the sequence, and its largest sub_* is the minor base"""
    c1 = synth.make_species(1, 600, 0.0, seed=67)[0].tobytes().decode()
    p = 311; minor = "ACGT"[("ACGT".index(c1[p]) + 2) % 4]
    c2 = c1[:p] + minor + c1[p + 1:]
    enc = lambda s: np.frombuffer(s.encode(), dtype=np.uint8)
    r1 = _rs(synth.make_reads([enc(c1)], 210, mu=17.0, seed=68, rc_fraction=0.5)); r2 = _rs(synth.make_reads([enc(c2)], 90, mu=17.0, seed=69, rc_fraction=0.5))
    rs = _concat([r1, r2])
    got = _same(gpu_api, oracle, [c1], rs, np.array([0, 300], dtype=np.uint64), what="planted variant")
    cnt = got[0].astype(np.float64)
    assert int(np.argmin(cnt[:, 1] / cnt[:, 0])) == p
    assert "ACGT"[int(np.argmax(cnt[p, 2:6]))] == minor and cnt[p, 2 + "ACGT".index(minor)] > 60


def test_pipeline_samples_equal_single_runs(gpu_api):
    sp = synth.make_species(3, 500, 0.12, seed=71)
    parts = []
    for s, n in enumerate((500, 300)):
        rs0 = _rs(synth.make_reads(sp, n, mu=15.0, seed=72 + s, rc_fraction=0.2))
        score, err, keep = gpu_api.score_reads(rs0, 13, 7.0)
        idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
        parts.append((subset_reads(rs0, idx), score[idx]))
    seq = np.concatenate([p[0].seq for p in parts]); qual = np.concatenate([p[0].qual for p in parts])
    lens = np.concatenate([np.diff(p[0].off.astype(np.int64)) for p in parts]); off = np.zeros(len(lens) + 1, dtype=np.uint64); off[1:] = np.cumsum(lens)
    allrs = ReadSet(seq, qual, off); seg = np.array([0, parts[0][0].n, parts[0][0].n + parts[1][0].n], dtype=np.uint64)
    score = np.concatenate([p[1] for p in parts])
    kw = dict(KW, abundance_ratio=0.1)
    plain = pipeline.run_hot_path_samples(gpu_api, allrs, score, seg, **kw)
    both = pipeline.run_hot_path_samples(gpu_api, allrs, score, seg, support=True, **kw)
    for s, (rs, sc) in enumerate(parts):
        one = pipeline.run_hot_path(gpu_api, rs, sc, support=True, **kw)
        assert one["centers"] == both[s]["centers"] == plain[s]["centers"] and len(one["centers"]) >= 2
        assert "support" not in plain[s] and len(one["support"]) == len(both[s]["support"]) == len(one["centers"])
        for x, y in zip(one["support"], both[s]["support"]):
            assert np.array_equal(x, y) and x[:, 0].max() > 20


def _files(out):
    res = {}
    for root, _, fs in os.walk(out):
        for f in fs:
            res[os.path.relpath(os.path.join(root, f), out)] = open(os.path.join(root, f), "rb").read()
    return res


@pytest.mark.parametrize("extra", [["--racon", "--racon_iter", "2"], [], ["--racon", "--racon_iter", "1", "--remove_universal_tails"]])
def test_cli_flag(gpu_api, tmp_path, extra):
    from ngspeciesid_amd import cli as _cli, fastpath
    res = []
    for flag in ([], ["--consensus_support"]):
        out = str(tmp_path / ("o%d" % len(flag))); os.makedirs(out)
        args = _cli.build_parser().parse_args(["--ont", "--fastq", os.path.join(GOLD, "sample_h1.fastq"), "--outfolder", out, "--t", "1", "--consensus"] + extra + flag); args.k, args.w = 13, 20
        fastpath.main(args, api=gpu_api)
        res.append(_files(out))
    a, b = res
    assert set(a) <= set(b) and all(a[f] == b[f] for f in a if f != "logfile.txt")
    if "--racon" in extra:
        stems = sorted(f[:-len("consensus.fasta")] for f in a if f.endswith(os.path.join("", "consensus.fasta")))
        trip = [(d + "consensus.fasta", d + "consensus.fastq", d + "consensus_support.tsv") for d in stems]
    else:
        stems = sorted(f[:-len(".fasta")] for f in a if f.startswith("consensus_reference_"))
        trip = [(d + ".fasta", d + ".fastq", d + ".support.tsv") for d in stems]
    assert trip and sorted(set(b) - set(a)) == sorted(x for t in trip for x in t[1:])
    for fa, fq, tsv in trip:
        fal = b[fa].decode().split("\n"); fql = b[fq].decode().split("\n"); rows = b[tsv].decode().splitlines()
        assert fql[0] == "@" + fal[0][1:] and fql[1] == fal[1] and fql[2] == "+" and len(fql[3]) == len(fal[1]) and fql[4:] == [""]
        assert rows[0].split("\t") == ["pos", "base", "depth", "agree", "A", "C", "G", "T", "del", "ins_after"] and len(rows) == len(fal[1]) + 1
        tab = np.array([[int(v) for v in r.split("\t")[2:]] for r in rows[1:]])
        from ngspeciesid_amd import consensus
        assert fql[3] == (consensus.support_phred(tab) + 33).astype(np.uint8).tobytes().decode() and tab[:, 0].max() > 10


def test_cli_flag_under_fastq_dir(gpu_api, tmp_path):
    import shutil
    from ngspeciesid_amd import cli as _cli, fastpath
    d = tmp_path / "in"; d.mkdir()
    shutil.copy(os.path.join(GOLD, "sample_h1.fastq"), str(d / "h1.fastq"))
    synth.reads_to_fastq(synth.make_reads(synth.make_species(2, 600, 0.12, seed=81), 400, mu=15.0, seed=82, rc_fraction=0.3), str(d / "s_a.fastq"), prefix="a")
    res = []
    for flag in ([], ["--consensus_support"]):
        out = str(tmp_path / ("o%d" % len(flag))); os.makedirs(out)
        args = _cli.build_parser().parse_args(["--ont", "--fastq_dir", str(d), "--outfolder", out, "--t", "1", "--consensus", "--racon", "--racon_iter", "1"] + flag); args.k, args.w = 13, 20
        fastpath.main(args, api=gpu_api)
        res.append(_files(out))
    a, b = res
    assert set(a) <= set(b) and all(a[f] == b[f] for f in a if not f.endswith("logfile.txt"))
    stems = sorted(f[:-len("consensus.fasta")] for f in a if f.endswith(os.sep + "consensus.fasta"))
    assert {s.split(os.sep)[0] for s in stems} == {"h1", "s_a"}
    assert sorted(set(b) - set(a)) == sorted(s + n for s in stems for n in ("consensus.fastq", "consensus_support.tsv"))
    for s in stems:
        assert b[s + "consensus.fastq"].decode().split("\n")[1] == b[s + "consensus.fasta"].decode().split("\n")[1]
