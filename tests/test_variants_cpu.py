"""The policy layer of the variant table (ngspeciesid_amd/variants.py) on hand-written neighbour lists, against the plain-loop restatement of variants_reference.py.
No device: the neighbour lists are written out, or come from the reference's brute force through a stand-in for Api.near_pairs."""
import os
import argparse
import numpy as np
import pytest
import variants_reference as ref
import variants_cases as vc
from ngspeciesid_amd import variants
from ngspeciesid_amd._capi import NEAR_MAX_DIST


class RefApi:
    """Api.near_pairs by the reference's brute force"""
    def __init__(self): self.calls = []

    def near_pairs(self, seqs, max_dist, both_strands=True):
        strs = [seqs.get(i)[0] for i in range(seqs.n)]
        self.calls.append((len(strs), max_dist, both_strands))
        p = ref.near_pairs(strs, max_dist, both_strands)
        return tuple(np.array([r[k] for r in p], dtype=t) for k, t in enumerate((np.uint32, np.uint32, np.uint8, np.uint8)))


def _cluster(sizes, seqs, pairs, thr):
    """variants.cluster and the reference on the same neighbour list -> the library's result, after comparing"""
    lengths = [len(s) for s in seqs]
    pi = [p[0] for p in pairs]; pj = [p[1] for p in pairs]
    got = variants.cluster(sizes, lengths, seqs, (pi, pj), [p[2] for p in pairs], thr, [p[3] for p in pairs])
    want = ref.cluster(sizes, lengths, seqs, pairs, lambda i, j: max(thr[i], thr[j]))
    assert got[0].tolist() == want[0] and list(got[1]) == want[1] and got[2].tolist() == want[2] and got[3].tolist() == want[3]
    return got


def test_the_reference_agrees_with_itself():
    """the side-by-side rectangle of the brute force against the single one, and the known distances of the generators"""
    rng = np.random.default_rng(2)
    seqs = [vc.rand_seq(rng, int(n), "ACGTN") for n in (0, 1, 7, 30, 31, 64)] + [""]
    seqs += [vc.mutate(rng, seqs[3], 0.1), ref.rc(seqs[4])]
    for a in seqs:
        assert ref.ed_many(a, seqs).tolist() == [ref.ed(a, b) for b in seqs]
    assert ref.ed("", "ACG") == 3 and ref.ed("ACG", "") == 3 and ref.ed("N", "N") == 0 and ref.ed("N", "A") == 1 and ref.ed("ACGT", "AGT") == 1 and ref.ed("kitten".upper(), "sitting".upper()) == 3
    assert ref.D("AAAAC", "GTTTT") == (0, 1) and ref.D("ACGT", "ACGT") == (0, 0) and ref.rc("ACGTN") == "NACGT"
    for k in (0, 3, 9):
        assert ref.ed(*vc.at_distance(rng, 40, k)) == k
        for where in ("lead", "trail", "mid"):
            assert ref.ed(*vc.indel_only(rng, 40, k, where)) == k
    want = [(i, j, *ref.D(seqs[i], seqs[j])) for i in range(len(seqs)) for j in range(i + 1, len(seqs)) if ref.D(seqs[i], seqs[j])[0] <= 6]
    assert ref.near_pairs(seqs, 6) == want and (0, 6, 0, 0) in want


def test_thresholds_are_integer_arithmetic():
    t, K = variants.thresholds([600, 650, 100, 0, 2000], "0.97", 31)
    assert t.tolist() == [18, 19, 3, 0, 31] and K == 31
    assert variants.thresholds([600], "0.97", 5)[0].tolist() == [5]
    assert variants.thresholds([1000], "0.999", 31) == (np.array([1]), 1)
    assert variants.thresholds([100], "1", 31)[1] == 0 and variants.thresholds([10], "0", 31)[1] == 10 and variants.thresholds([100], "1.0", 31)[1] == 0
    assert variants.thresholds([], "0.97", 31)[1] == 0
    # 0.97 has no exact float: (1 - 0.97) * 100 = 3.0000000000000027 happens to round down right, (1 - 0.9) * 10 = 0.9999999999999998 does not
    assert variants.thresholds([10], "0.9", 31)[0].tolist() == [1] and int((1 - 0.9) * 10) == 0
    want = ref.thresholds([600, 650, 100, 0, 2000], "0.97", 31)
    assert [[want(i, j) for j in range(5)] for i in range(5)] == [[max(int(t[i]), int(t[j])) for j in range(5)] for i in range(5)]


def test_flag_errors():
    for ident, md, word in (("0.97", NEAR_MAX_DIST + 1, "--variant_max_dist"), ("0.97", -1, "--variant_max_dist"), ("1.2", 31, "--variant_identity"),
                            ("abc", 31, "--variant_identity"), ("0.", 31, "--variant_identity"), ("-0.5", 31, "--variant_identity")):
        with pytest.raises(ValueError) as e:
            variants.thresholds([100], ident, md)
        assert word in str(e.value), (ident, md, str(e.value))
        assert word in variants.check_args(argparse.Namespace(variant_identity=ident, variant_max_dist=md))
    assert variants.check_args(argparse.Namespace(variant_identity="0.97", variant_max_dist=31)) is None
    p = argparse.ArgumentParser(); variants.add_flags(p)
    a = p.parse_args([])
    assert (a.variant_identity, a.variant_max_dist, a.variant_one_strand) == ("0.97", 31, False)


def test_cli_refuses_variants_without_samples_or_consensus(tmp_path, caplog):
    from ngspeciesid_amd.cli import cli
    fq = tmp_path / "r.fastq"; fq.write_text("@r\nACGT\n+\nIIII\n")
    d = tmp_path / "d"; d.mkdir()
    for flags, word in ((["--fastq", str(fq), "--consensus", "--variants"], "--fastq_dir or --demux_sheet"),
                        (["--fastq_dir", str(d), "--t", "1", "--variants"], "--consensus"),
                        (["--fastq_dir", str(d), "--t", "1", "--consensus", "--variants", "--variant_max_dist", "32"], "--variant_max_dist")):
        caplog.clear()
        with pytest.raises(SystemExit) as e:
            cli(["--ont", "--outfolder", str(tmp_path / "o")] + flags)
        assert e.value.code == 1 and word in caplog.text, (flags, caplog.text)
    with pytest.raises(SystemExit) as e:
        cli(["variants", "--fasta", str(tmp_path / "missing.fasta"), "--outfolder", str(tmp_path / "o")])
    assert e.value.code == 1


def test_chain_and_centroids_only():
    """a - b - c with a - c over the threshold: b joins a, and c founds its own variant because b is no centroid"""
    seqs = ["A" * 100, "A" * 99 + "C", "A" * 98 + "CC"]
    pairs = [(0, 1, 1, 0), (1, 2, 1, 0), (0, 2, 2, 0)]
    vo, cents, md, ms = _cluster([30, 20, 10], seqs, pairs, [1, 1, 1])
    assert vo.tolist() == [0, 0, 1] and cents == [0, 2] and md.tolist() == [0, 1, 0]
    # with b the most abundant, both neighbours join it
    vo, cents, md, _ = _cluster([20, 30, 10], seqs, pairs, [1, 1, 1])
    assert vo.tolist() == [0, 0, 0] and cents == [1] and md.tolist() == [1, 0, 1]
    # the threshold of a pair is that of its longer sequence
    vo, _, _, _ = _cluster([30, 20], ["A" * 10, "A" * 50], [(0, 1, 3, 0)], [0, 3])
    assert vo.tolist() == [0, 0]
    vo, _, _, _ = _cluster([30, 20], ["A" * 10, "A" * 50], [(0, 1, 3, 0)], [0, 2])
    assert vo.tolist() == [0, 1]


def test_every_tie_in_the_centroid_order():
    # reads descending
    assert _cluster([5, 9], ["AAAA", "AAAC"], [(0, 1, 1, 0)], [1, 1])[1] == [1]
    # equal reads: the longer one first
    assert _cluster([5, 5], ["AAAA", "AAAAC"], [(0, 1, 1, 0)], [1, 1])[1] == [1]
    # equal reads and length: the smaller bytes first
    assert _cluster([5, 5], ["AAAC", "AAAA"], [(0, 1, 1, 0)], [1, 1])[1] == [1]
    # identical sequences with equal reads: the smaller index
    vo, cents, md, _ = _cluster([5, 5], ["AAAA", "AAAA"], [(0, 1, 0, 0)], [0, 0])
    assert cents == [0] and vo.tolist() == [0, 0] and md.tolist() == [0, 0]
    # a sequence within reach of two centroids joins the one founded first, not the nearer one
    seqs = ["A" * 40, "C" * 40, "A" * 20 + "C" * 20]
    vo, cents, md, _ = _cluster([9, 8, 1], seqs, [(0, 2, 5, 0), (1, 2, 2, 1)], [5, 5, 5])
    assert cents == [0, 1] and vo.tolist() == [0, 1, 0] and md.tolist() == [0, 0, 5]


def _groups(rng, n_samples=4):
    """a few samples over three families 12 % apart; one sample holds its sequences reverse-complemented"""
    roots = [vc.rand_seq(rng, 120) for _ in range(3)]
    groups = []
    for s in range(n_samples):
        cons = []
        for f in rng.permutation(3)[:int(rng.integers(1, 4))]:
            q = vc.mutate(rng, roots[int(f)], 0.02)
            if s == 1: q = ref.rc(q)
            cons.append(("consensus_cl_id_%d_total_supporting_reads_%d" % (len(cons) * 7, 10 + 3 * s + int(f)), 10 + 3 * s + int(f), q))
        groups.append(("sample_%d" % s, None, cons))
    return groups


def _by_sequence(tab, col):
    """what must not depend on the order of the samples: per sequence its variant's centroid sequence, distance and strand; per variant its row by sample name"""
    cent = {v["name"]: v["seq"] for v in tab["variants"]}
    members = {(m["sample"], m["consensus id"]): (cent[m["variant"]], m["dist"], m["strand"]) for m in tab["members"]}
    rows = {v["seq"]: dict(zip(tab["samples"], row.tolist())) for v, row in zip(tab["variants"], tab["counts"])}
    return members, rows, [v["seq"] for v in tab["variants"]]


def test_order_independence_strands_and_sums():
    rng = np.random.default_rng(11)
    groups = _groups(rng)
    api = RefApi()
    col = variants.collect(groups)
    tab = variants.build(api, col, identity="0.9", max_dist=31)
    assert api.calls == [(len(col["seqs"]), 12, True)]                          # one call, with the largest threshold any pair can need
    assert len(tab["variants"]) == 3 and tab["counts"].sum() == col["sizes"].sum()
    assert tab["counts"].sum(axis=1).tolist() == [v["size"] for v in tab["variants"]]
    for s, name in enumerate(tab["samples"]):
        assert tab["counts"][:, s].sum() == sum(nr for _, nr, _ in groups[s][2])
    # a member is on strand '-' exactly when one of it and its centroid comes from the reverse-complemented sample
    flipped = [m["sample"] == "sample_1" for m in tab["members"]]
    cent_of = {v["name"]: col["seqs"].index(v["seq"]) for v in tab["variants"]}
    assert [m["strand"] for m in tab["members"]] == ["-" if flipped[x] != flipped[cent_of[m["variant"]]] else "+" for x, m in enumerate(tab["members"])]
    assert "-" in [m["strand"] for m in tab["members"]]
    want = _by_sequence(tab, col)
    for perm in ([3, 2, 1, 0], [1, 3, 0, 2]):
        g2 = [groups[p] for p in perm]
        c2 = variants.collect(g2)
        t2 = variants.build(RefApi(), c2, identity="0.9", max_dist=31)
        assert _by_sequence(t2, c2) == want, perm
    one = variants.build(RefApi(), col, identity="0.9", max_dist=31, both_strands=False)
    assert len(one["variants"]) > 3                                             # without the reverse strand the flipped sample stands alone


def test_write_then_read_round_trips(tmp_path):
    rng = np.random.default_rng(5)
    groups = _groups(rng, 3)
    col = variants.collect(groups)
    tab = variants.build(RefApi(), col, identity="0.9", max_dist=31)
    variants.write(str(tmp_path), tab)
    assert sorted(os.listdir(tmp_path)) == ["variant_members.tsv", "variant_table.tsv", "variants.fasta"]
    rows = variants.read_table(str(tmp_path / "variant_table.tsv"))
    assert [r["variant"] for r in rows] == [v["name"] for v in tab["variants"]]
    assert [[r[s] for s in tab["samples"]] for r in rows] == tab["counts"].tolist()
    assert variants.read_table(str(tmp_path / "variant_members.tsv")) == tab["members"]
    assert open(tmp_path / "variant_members.tsv").readline() == "#sample\tconsensus id\treads\tvariant\tdist\tstrand\n"
    # variants.fasta is a plain FASTA the library reader of `classify --fasta` takes
    from ngspeciesid_amd import classify
    lib = classify.read_reference_fasta(str(tmp_path / "variants.fasta"), unique_names=False)
    assert [lib.rs.get(i)[0] for i in range(lib.rs.n)] == [v["seq"] for v in tab["variants"]]
    assert lib.headers == ["%s;size=%d;samples=%d" % (v["name"], v["size"], v["n_samples"]) for v in tab["variants"]]


def test_subcommand_sizes_and_names(tmp_path):
    """every FASTA one sample; sizes from this tool's headers, 1 elsewhere"""
    a, b = vc.rand_seq(np.random.default_rng(1), 60), vc.rand_seq(np.random.default_rng(2), 60)
    (tmp_path / "s1.fasta").write_text(">consensus_cl_id_4_total_supporting_reads_25\n%s\n>other\n%s\n" % (a, b))
    (tmp_path / "s2.fa").write_text(">x\n%s\n" % ref.rc(a))
    args = argparse.Namespace(fasta=[str(tmp_path / "s1.fasta"), str(tmp_path / "s2.fa")], outfolder=str(tmp_path / "out"), variant_identity="0.97", variant_max_dist=31, variant_one_strand=False)
    tab = variants.variants_fasta(args, api=RefApi())
    assert tab["samples"] == ["s1", "s2"] and tab["counts"].tolist() == [[25, 1], [1, 0]]
    assert [m["strand"] for m in tab["members"]] == ["+", "+", "-"] and [m["reads"] for m in tab["members"]] == [25, 1, 1]
    assert variants.read_table(str(tmp_path / "out" / "variant_members.tsv")) == tab["members"]
    args.fasta = [str(tmp_path / "s1.fasta"), str(tmp_path / "s1.fasta")]
    with pytest.raises(ValueError):
        variants.variants_fasta(args, api=RefApi())
