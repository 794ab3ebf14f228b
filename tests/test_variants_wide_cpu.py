"""The wide edit bound of the variant table (--variant_wide_max_dist; ngspeciesid_amd/variants.py) without a device: Api.near_pairs_wide is the reference's brute force
(variants_reference.py), and every table is held against the reference's plain-loop policy."""
import argparse
import numpy as np
import pytest
import variants_reference as ref
import variants_cases as vc
from ngspeciesid_amd import variants
from ngspeciesid_amd._capi import NEAR_MAX_DIST, NEAR_WIDE_MAX_DIST


class RefApi:
    """Api.near_pairs and Api.near_pairs_wide by the reference's brute force; `calls` says which one was used"""
    def __init__(self): self.calls = []

    def _pairs(self, which, seqs, max_dist, both_strands):
        strs = [seqs.get(i)[0] for i in range(seqs.n)]
        self.calls.append((which, len(strs), max_dist, both_strands))
        p = ref.near_pairs(strs, max_dist, both_strands)
        return tuple(np.array([r[k] for r in p], dtype=t) for k, t in enumerate((np.uint32, np.uint32, np.uint8, np.uint8)))

    def near_pairs(self, seqs, max_dist, both_strands=True): return self._pairs("near_pairs", seqs, max_dist, both_strands)

    def near_pairs_wide(self, seqs, max_dist, both_strands=True): return self._pairs("near_pairs_wide", seqs, max_dist, both_strands)


def test_thresholds_with_the_wide_bound():
    assert NEAR_WIDE_MAX_DIST > NEAR_MAX_DIST
    t, K = variants.thresholds([1500, 4500, 650, 0], "0.97", 31, wide_max_dist=NEAR_WIDE_MAX_DIST)
    assert t.tolist() == [45, 135, 19, 0] and K == 135
    assert variants.thresholds([1500], "0.97", 31, wide_max_dist=40) == (np.array([40]), 40)
    assert variants.thresholds([650], "0.90", 31, wide_max_dist=NEAR_WIDE_MAX_DIST)[1] == 65
    assert variants.thresholds([16384], "0.9", 31, wide_max_dist=NEAR_WIDE_MAX_DIST)[1] == NEAR_WIDE_MAX_DIST
    # the wide bound replaces --variant_max_dist: that one is not looked at, and without the wide bound nothing changes
    assert variants.thresholds([1500], "0.97", 5, wide_max_dist=60)[1] == 45 and variants.thresholds([1500], "0.97", 5)[1] == 5
    assert variants.thresholds([1500], "0.97", 31, wide_max_dist=None)[1] == 31 and variants.thresholds([1500], "0.97", 31, wide_max_dist=0)[1] == 0
    want = ref.thresholds([1500, 4500, 650, 0], "0.97", NEAR_WIDE_MAX_DIST)
    assert [[want(i, j) for j in range(4)] for i in range(4)] == [[max(int(t[i]), int(t[j])) for j in range(4)] for i in range(4)]


def test_range_errors_name_the_new_flag():
    for wide in (NEAR_WIDE_MAX_DIST + 1, -1):
        with pytest.raises(ValueError) as e:
            variants.thresholds([100], "0.97", 31, wide_max_dist=wide)
        assert "--variant_wide_max_dist" in str(e.value)
        assert "--variant_wide_max_dist" in variants.check_args(argparse.Namespace(variant_identity="0.97", variant_max_dist=31, variant_wide_max_dist=wide))
        with pytest.raises(ValueError):
            variants.build(RefApi(), variants.collect([("s", None, [("a", 1, "ACGT"), ("b", 1, "ACGA")])]), wide_max_dist=wide)
    assert variants.check_args(argparse.Namespace(variant_identity="0.97", variant_max_dist=31, variant_wide_max_dist=NEAR_WIDE_MAX_DIST)) is None
    assert variants.check_args(argparse.Namespace(variant_identity="0.97", variant_max_dist=31, variant_wide_max_dist=None)) is None
    assert variants.check_args(argparse.Namespace(variant_identity="0.97", variant_max_dist=31)) is None               # a namespace from before the flag
    # without the wide bound 32 is still refused under the old flag's name, and the text points to the new one
    text = variants.check_args(argparse.Namespace(variant_identity="0.97", variant_max_dist=NEAR_MAX_DIST + 1, variant_wide_max_dist=None))
    assert "--variant_max_dist" in text and "--variant_wide_max_dist" in text
    # with it, --variant_max_dist is not looked at
    assert variants.check_args(argparse.Namespace(variant_identity="0.97", variant_max_dist=NEAR_MAX_DIST + 1, variant_wide_max_dist=40)) is None


def test_the_flag_parses_on_both_parsers():
    from ngspeciesid_amd import cli
    p = argparse.ArgumentParser(); variants.add_flags(p)
    assert p.parse_args([]).variant_wide_max_dist is None and p.parse_args(["--variant_wide_max_dist", "80"]).variant_wide_max_dist == 80
    sub = cli._variants_subparser(argparse.ArgumentParser(prog="variants"))
    a = sub.parse_args(["--fasta", "x.fasta", "--outfolder", "o", "--variant_wide_max_dist", "135"])
    assert a.variant_wide_max_dist == 135 and a.variant_max_dist == NEAR_MAX_DIST
    assert sub.parse_args(["--fasta", "x.fasta", "--outfolder", "o"]).variant_wide_max_dist is None
    assert variants._kwargs(a)["wide_max_dist"] == 135


def test_the_main_command_takes_and_checks_the_flag(tmp_path, caplog):
    from ngspeciesid_amd.cli import cli
    d = tmp_path / "d"; d.mkdir()
    with pytest.raises(SystemExit) as e:
        cli(["--ont", "--outfolder", str(tmp_path / "o"), "--fastq_dir", str(d), "--t", "1", "--consensus", "--variants", "--variant_wide_max_dist", str(NEAR_WIDE_MAX_DIST + 1)])
    assert e.value.code == 1 and "--variant_wide_max_dist" in caplog.text


def _two_templates(rng, n_samples=3):
    """every sample holds a copy of each of two 700-base templates that are 8 % apart (substitutions only, so exactly 56 edits on equal lengths), each with a few
    edits of its own -> groups"""
    a = vc.rand_seq(rng, 700)
    b = list(a)
    for p in rng.choice(700, size=56, replace=False): b[int(p)] = "ACGT"[("ACGT".index(b[int(p)]) + 1 + int(rng.integers(0, 3))) % 4]
    b = "".join(b)
    groups = []
    for s in range(n_samples):
        cons = []
        for f, root in enumerate((a, b)):
            q = root if s == 0 else vc.mutate(rng, root, 0.004)
            if s == 1: q = ref.rc(q)
            cons.append(("consensus_cl_id_%d_total_supporting_reads_%d" % (f, 40 - 10 * s - 3 * f), 40 - 10 * s - 3 * f, q))
        groups.append(("sample_%d" % s, None, cons))
    return groups


def _reference_table(col, identity, K, both=True):
    lengths = [len(s) for s in col["seqs"]]
    return ref.cluster(col["sizes"], lengths, col["seqs"], ref.near_pairs(col["seqs"], K, both), ref.thresholds(lengths, identity, K))


def test_build_joins_beyond_31_edits_only_with_the_wide_bound():
    rng = np.random.default_rng(17)
    col = variants.collect(_two_templates(rng))
    assert 40 < ref.ed(col["seqs"][0], col["seqs"][1]) <= 56
    api = RefApi()
    wide = variants.build(api, col, identity="0.9", wide_max_dist=80)
    K = max((10 * len(s)) // 100 for s in col["seqs"])
    assert api.calls == [("near_pairs_wide", 6, K, True)] and 69 <= K <= 71                        # one call, the wide one, with the largest threshold any pair can need
    assert len(wide["variants"]) == 1 and wide["variants"][0]["n_samples"] == 3 and wide["counts"].sum() == col["sizes"].sum()
    want = _reference_table(col, "0.9", 80)
    assert wide["variant_of"].tolist() == want[0] and wide["dist"].tolist() == want[2] and wide["strand"].tolist() == want[3]
    assert max(want[2]) > NEAR_MAX_DIST and 1 in want[3]
    api = RefApi()
    narrow = variants.build(api, col, identity="0.9")
    assert api.calls == [("near_pairs", 6, NEAR_MAX_DIST, True)]
    assert len(narrow["variants"]) == 2 and narrow["variant_of"].tolist() == _reference_table(col, "0.9", NEAR_MAX_DIST)[0]
    # a wide bound below 32 is legal and goes through the wide call as well
    api = RefApi()
    small = variants.build(api, col, identity="0.9", wide_max_dist=NEAR_MAX_DIST)
    assert api.calls[0][0] == "near_pairs_wide" and small["variant_of"].tolist() == narrow["variant_of"].tolist()


def test_the_subcommand_writes_the_three_files(tmp_path):
    rng = np.random.default_rng(23)
    groups = _two_templates(rng)
    paths = []
    for name, _, cons in groups:
        paths.append(str(tmp_path / (name + ".fasta")))
        with open(paths[-1], "w") as fh:
            for cid, _, q in cons: fh.write(">%s\n%s\n" % (cid, q))
    args = argparse.Namespace(fasta=paths, outfolder=str(tmp_path / "out"), variant_identity="0.9", variant_max_dist=31, variant_one_strand=False, variant_wide_max_dist=80)
    api = RefApi()
    tab = variants.variants_fasta(args, api=api)
    assert [c[0] for c in api.calls] == ["near_pairs_wide"]
    col = variants.collect(groups)
    want = _reference_table(col, "0.9", 80)
    assert tab["variant_of"].tolist() == want[0] and tab["dist"].tolist() == want[2] and tab["strand"].tolist() == want[3] and len(want[1]) == 1
    members = variants.read_table(str(tmp_path / "out" / "variant_members.tsv"))
    assert members == tab["members"] and [m["dist"] for m in members] == want[2] and [m["strand"] for m in members] == ["+-"[s] for s in want[3]]
    assert open(tmp_path / "out" / "variant_members.tsv").readline() == "#sample\tconsensus id\treads\tvariant\tdist\tstrand\n"
    rows = variants.read_table(str(tmp_path / "out" / "variant_table.tsv"))
    assert [[r[s] for s in tab["samples"]] for r in rows] == [[sum(nr for _, nr, _ in g[2]) for g in groups]]
    assert open(tmp_path / "out" / "variants.fasta").read() == ">variant_0;size=%d;samples=3\n%s\n" % (int(col["sizes"].sum()), col["seqs"][want[1][0]])
    # the same files without the flag: the two templates stay apart
    args.variant_wide_max_dist = None; args.outfolder = str(tmp_path / "out2")
    assert len(variants.variants_fasta(args, api=RefApi())["variants"]) == 2
