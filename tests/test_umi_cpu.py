"""The policy layer of the UMI mode (ngspeciesid_amd/umi.py) against the plain-loop restatement of umi_reference.py, and ngsid_umi_centroids (a host function of the
library) against variants_reference.cluster.  No device: flanks are located by the host locator, pairs come from brute force, the consensus from the CPU oracle."""
import argparse
import functools
import os
import numpy as np
import pytest
import variants_reference as vr
import variants_cases as vc
import demux_reference as dr
import umi_reference as ur
import umi_cases as uc
from ngspeciesid_amd import umi, runtime
from ngspeciesid_amd._capi import Api, ReadSet, NgsidError, UMI_MAX_DIST

DESIGN = umi.Design(*uc.FLANKS, umi_len=uc.UMI_LEN, len_slack=uc.LEN_SLACK)


class RefApi:
    """Api.demux_locate by the host locator, Api.umi_pairs by brute force, Api.umi_centroids by the library's host function, consensus calls by the CPU oracle"""
    def __init__(self, oracle=None):
        self.host = Api(runtime.load_library(), "ngsid_", None); self.oracle = oracle; self.calls = []

    def demux_locate(self, rs, tags, window=150, max_ed=3, iupac=True):
        return dr.locate([rs.get(i)[0] for i in range(rs.n)], list(tags), window, max_ed, iupac)[0]

    def umi_pairs(self, seqs, max_dist, seed_len):
        strs = [seqs.get(i)[0] for i in range(seqs.n)]
        self.calls.append((len(strs), max_dist, seed_len))
        p = ur.pairs(strs, max_dist)
        return tuple(np.array([r[k] for r in p], dtype=t) for k, t in enumerate((np.uint32, np.uint32, np.uint8)))

    def umi_centroids(self, pi, pj, order):
        return self.host.umi_centroids(pi, pj, order)

    def poa_consensus(self, *a, **kw): return self.oracle.poa_consensus(*a, **kw)
    def polish(self, *a, **kw): return self.oracle.polish(*a, **kw)


@functools.lru_cache(maxsize=None)
def _run():
    return uc.make_run(5)


def _rs(run):
    return ReadSet.from_strings(run["seqs"], run["quals"])


def _check_extract(got, want):
    names = {umi.ST_OK: "ok", umi.ST_NO_UMI: "no_umi", umi.ST_BAD_LEN: "bad_len"}
    for r, w in enumerate(want):
        g = (names[int(got["status"][r])], {0: "+", 1: "-", -1: None}[int(got["strand"][r])], got["key"][r], int(got["cut0"][r]), int(got["cut1"][r]))
        assert g == w, (r, g, w)


def test_extract_orientation_statuses_and_one_key_per_molecule():
    run = _run()
    got = umi.extract(RefApi(), _rs(run), DESIGN, 150, 3)
    _check_extract(got, ur.extract(run["seqs"], uc.FLANKS, uc.UMI_LEN, uc.LEN_SLACK, 150, 3))
    has = run["molecule"] >= 0
    assert (got["status"][has] == umi.ST_OK).all() and (got["strand"][has] == run["strand"][has]).all() and 0 < run["strand"][has].sum() < has.sum()
    assert sorted(got["status"][~has].tolist()) == [umi.ST_NO_UMI] * 3 + [umi.ST_BAD_LEN] * 3
    # at most one planted edit per key: the key of every read is within one edit of its molecule's, on either strand
    for r in np.flatnonzero(has):
        uf, urv = run["umis"][int(run["molecule"][r])]
        assert vr.ed(got["key"][r], uf + urv) <= 1, r
    # the amplicon between the inner cuts, oriented, is the read's copy of its template: closer to it than to any other
    work = umi.trimmed_oriented(_rs(run), got)
    for r in np.flatnonzero(has)[:20]:
        t = run["template_of"][int(run["molecule"][r])]
        assert vr.ed(work.get(int(r))[0], run["templates"][t]) <= 12


def test_both_strands_of_a_molecule_give_the_same_key_and_ties_go_to_plus():
    rng = np.random.default_rng(3)
    fp, fq, rp, rq = uc.FLANKS
    uf, urv = vc.rand_seq(rng, 18), vc.rand_seq(rng, 18)
    read = "ACGT" + fp + uf + fq + vc.rand_seq(rng, 200) + dr.revcomp(rp + urv + rq) + "TT"
    # a palindromic design (the reverse flanks are the forward ones): both orientations hold with equal distances
    sym = fp + uf + fq + vc.rand_seq(rng, 100) + dr.revcomp(fp + urv + fq)
    pal = umi.Design(fp, fq, fp, fq, 18, 2)
    api = RefApi()
    got = umi.extract(api, ReadSet.from_strings([read, dr.revcomp(read)]), DESIGN, 150, 3)
    assert got["key"] == [uf + urv] * 2 and got["strand"].tolist() == [0, 1] and got["status"].tolist() == [0, 0]
    assert (int(got["cut0"][0]), int(got["cut1"][0])) == (4 + 20 + 18 + 20, 2 + 20 + 18 + 20) and (int(got["cut0"][1]), int(got["cut1"][1])) == (2 + 58, 4 + 58)
    got = umi.extract(api, ReadSet.from_strings([sym]), pal, 150, 3)
    assert got["strand"].tolist() == [0] and got["key"] == [uf + urv]
    _check_extract(got, ur.extract([sym], (fp, fq, fp, fq), 18, 2, 150, 3))
    # a UMI three letters too long at one end; a read without its reverse flanks
    long_ = fp + uf + "ACG" + fq + vc.rand_seq(rng, 100) + dr.revcomp(rp + urv + rq)
    bare = fp + uf + fq + vc.rand_seq(rng, 200)
    got = umi.extract(api, ReadSet.from_strings([long_, bare, ""]), DESIGN, 150, 3)
    assert got["status"].tolist() == [umi.ST_BAD_LEN, umi.ST_NO_UMI, umi.ST_NO_UMI] and got["key"] == [None] * 3


def test_reference_bins_are_the_molecules():
    """what the generator promises: keys of one molecule at most 2 apart, keys of two molecules far apart, so the reference's bins are the molecules"""
    run = _run()
    ex = ur.extract(run["seqs"], uc.FLANKS, uc.UMI_LEN, uc.LEN_SLACK, 150, 3)
    keys = [e[2] for e in ex]
    rbin, rows, small = ur.bins(keys, 3, 3)
    mol = run["molecule"]
    assert len(rows) == len(run["umis"]) and not any(small)
    for m in range(len(run["umis"])):
        mine = {rbin[r] for r in np.flatnonzero(mol == m)}
        assert len(mine) == 1 and -1 not in mine
        ks = [keys[r] for r in np.flatnonzero(mol == m)]
        assert max(vr.ed(a, b) for a in ks for b in ks) <= 2
    assert len({rbin[r] for r in np.flatnonzero(mol >= 0)}) == len(run["umis"])


def test_bins_equal_the_reference_and_ignore_input_order():
    run = _run()
    api = RefApi()
    ex = umi.extract(api, _rs(run), DESIGN, 150, 3)
    bn = umi.bins(api, ex["key"], 3, 3, DESIGN)
    assert api.calls == [(len(bn["umis"]), 3, 8)]                                 # one call; 2 * (18 - 2) // 4 = 8
    rbin, rows, small = ur.bins(ex["key"], 3, 3)
    got_bin = np.where(bn["key_of"] >= 0, bn["bin_of"][np.maximum(bn["key_of"], 0)], -1)
    assert got_bin.tolist() == rbin and small == bn["small"].tolist()
    assert rows == [(bn["umis"][c], int(bn["reads"][b]), int(bn["distinct"][b])) for b, c in enumerate(bn["centroids"])]
    for x, k in enumerate(bn["umis"]):
        assert bn["dist"][x] == vr.ed(k, bn["umis"][bn["centroids"][bn["bin_of"][x]]])
    perm = np.random.default_rng(1).permutation(len(ex["key"]))
    b2 = umi.bins(RefApi(), [ex["key"][p] for p in perm], 3, 3, DESIGN)
    assert b2["umis"] == bn["umis"] and b2["bin_of"].tolist() == bn["bin_of"].tolist() and b2["centroids"] == bn["centroids"]
    # min_reads: with 7 every bin of six reads is small
    assert umi.bins(RefApi(), ex["key"], 3, 7, DESIGN)["small"].all()
    empty = umi.bins(RefApi(), [None, None], 3, 3, DESIGN)
    assert empty["umis"] == [] and empty["centroids"] == [] and empty["key_of"].tolist() == [-1, -1]


def test_seed_len_policy():
    assert [umi.seed_len(DESIGN, d) for d in range(9)] == [16, 16, 10, 8, 6, 5, 4, 4, 4]
    assert umi.seed_len(umi.Design("A", "C", "G", "T", 5, 2), 3) == 4


def test_centroids_equal_the_reference_on_random_graphs():
    host = Api(runtime.load_library(), "ngsid_", None)
    rng = np.random.default_rng(8)
    for trial in range(30):
        n = int(rng.integers(1, 60))
        m = int(rng.integers(0, 3 * n))
        pairs = [(int(a), int(b)) for a, b in rng.integers(0, n, (m, 2)) if a != b]
        pairs += [(k, k + 1) for k in range(0, n - 1, 3)]                          # chains
        pairs += pairs[:3]                                                        # a pair listed twice counts once
        order = rng.permutation(n)
        got_bin, got_cent = host.umi_centroids([p[0] for p in pairs], [p[1] for p in pairs], order)
        want_bin, want_cent = ur.centroids(pairs, order.tolist(), n)
        assert got_bin.tolist() == want_bin and got_cent.tolist() == want_cent, trial
    # a - b - c: walked a, b, c: b joins a and c founds its own bin, because b is no centroid; walked b first, both join it
    assert [x.tolist() for x in host.umi_centroids([0, 1], [1, 2], [0, 1, 2])] == [[0, 0, 1], [0, 2]]
    assert [x.tolist() for x in host.umi_centroids([0, 1], [1, 2], [1, 0, 2])] == [[0, 0, 0], [1]]
    # a node within reach of two centroids joins the one founded first
    assert [x.tolist() for x in host.umi_centroids([0, 1], [2, 2], [1, 0, 2])] == [[1, 0, 0], [1, 0]]
    assert [x.tolist() for x in host.umi_centroids([], [], [])] == [[], []]
    for bad in (([0], [0], [0, 1]), ([0], [2], [0, 1]), ([0], [1], [0, 0]), ([0], [1], [0, 2])):
        with pytest.raises(NgsidError):
            host.umi_centroids(*bad)


def test_flag_errors():
    p = argparse.ArgumentParser(); umi.add_flags(p)
    base = ["--umi_fwd", "ACGTACGT,GGTTGGTT", "--umi_rev", "CCAACCAA,TTGGTTGG"]
    a = p.parse_args(base)
    assert (a.umi_len, a.umi_len_slack, a.umi_max_dist, a.umi_flank_max_ed, a.umi_window, a.umi_min_reads, a.racon_iter) == (18, 2, 3, 3, 150, 3, 3)
    assert umi.check_args(a) is None and umi.design_of(a).flanks() == ["ACGTACGT", "GGTTGGTT", "CCAACCAA", "TTGGTTGG"]
    for extra, word in ((["--umi_max_dist", str(UMI_MAX_DIST + 1)], "--umi_max_dist"), (["--umi_max_dist", "-1"], "--umi_max_dist"), (["--umi_len", "31"], "--umi_len"),
                        (["--umi_len_slack", "18"], "--umi_len_slack"), (["--umi_window", "0"], "--umi_window"), (["--umi_window", "257"], "--umi_window"),
                        (["--umi_min_reads", "0"], "--umi_min_reads"), (["--umi_flank_max_ed", "-1"], "--umi_flank_max_ed"), (["--racon_iter", "-1"], "--racon_iter")):
        assert word in umi.check_args(p.parse_args(base + extra)), extra
    for fwd, word in (("ACGT", "--umi_fwd"), ("ACGT,acgt", "alphabet"), ("ACGT,", "alphabet"), ("A" * 65 + ",ACGT", "longer")):
        assert word in umi.check_args(p.parse_args(["--umi_fwd", fwd, "--umi_rev", "CCAA,TTGG"])), fwd
    with pytest.raises(ValueError):
        umi.bins(RefApi(), ["ACGT"], UMI_MAX_DIST + 1, 3, DESIGN)


def test_cli_refuses_bad_umi_flags(tmp_path, caplog):
    from ngspeciesid_amd.cli import cli
    fq = tmp_path / "r.fastq"; fq.write_text("@r\nACGT\n+\nIIII\n")
    for flags, word in ((["--umi_max_dist", "9"], "--umi_max_dist"), (["--umi_len", "40"], "--umi_len")):
        caplog.clear()
        with pytest.raises(SystemExit) as e:
            cli(["umi", "--fastq", str(fq), "--outfolder", str(tmp_path / "o"), "--umi_fwd", "ACGTACGT,GGTTGGTT", "--umi_rev", "CCAACCAA,TTGGTTGG"] + flags)
        assert e.value.code == 1 and word in caplog.text, (flags, caplog.text)
    with pytest.raises(SystemExit) as e:
        cli(["umi", "--fastq", str(tmp_path / "missing.fastq"), "--outfolder", str(tmp_path / "o"), "--umi_fwd", "ACGTACGT,GGTTGGTT", "--umi_rev", "CCAACCAA,TTGGTTGG"])
    assert e.value.code == 1


def test_oracle_consensus_of_every_bin_is_its_template_and_files_round_trip(oracle, tmp_path):
    """the end-to-end case of the GPU file on the CPU oracle: at the generator's error rate the polished consensus of every bin equals its template"""
    run = _run()
    res = umi.run(RefApi(oracle), _rs(run), DESIGN, window=150, flank_max_ed=3, max_dist=3, min_reads=3, racon_iter=3)
    bn = res["bins"]
    assert len(res["kept"]) == len(run["umis"]) == len(res["polished"])
    for b, seq in zip(res["kept"], res["polished"]):
        reads = np.flatnonzero(res["bin"] == b)
        mols = {int(run["molecule"][r]) for r in reads}
        assert len(mols) == 1 and len(reads) == 6
        assert seq == run["templates"][run["template_of"][mols.pop()]], b
    assert (res["status"][run["molecule"] >= 0] == umi.ST_OK).all()
    # with min_reads above the bin size nothing gets a consensus and every read with a key is small_bin
    small = umi.run(RefApi(oracle), _rs(run), DESIGN, min_reads=7)
    assert small["kept"] == [] and small["polished"] == [] and (small["status"][run["molecule"] >= 0] == umi.ST_SMALL_BIN).all()
    umi.write(str(tmp_path), run["names"], res)
    assert sorted(os.listdir(tmp_path)) == ["umi_bins.tsv", "umi_consensus.fasta", "umi_reads.tsv", "umi_summary.tsv"]
    rows = umi.read_table(str(tmp_path / "umi_bins.tsv"))
    assert rows == [dict(bin="umi_%d" % b, umi=bn["umis"][c], reads=int(bn["reads"][b]), distinct=int(bn["distinct"][b]), length=len(res["polished"][res["kept"].index(b)]))
                    for b, c in enumerate(bn["centroids"])]
    reads = umi.read_table(str(tmp_path / "umi_reads.tsv"))
    assert [r["read"] for r in reads] == run["names"] and [r["status"] for r in reads] == [umi.STATUS_NAMES[int(s)] for s in res["status"]]
    assert [r["bin"] for r in reads] == ["umi_%d" % b if b >= 0 else "." for b in res["bin"].tolist()] and [r["dist"] for r in reads] == res["dist"].tolist()
    assert [r["strand"] for r in reads] == [{0: "+", 1: "-", -1: "."}[int(s)] for s in res["extract"]["strand"]]
    assert open(tmp_path / "umi_reads.tsv").readline() == "#read\tstatus\tstrand\tumi\tbin\tdist\n" and open(tmp_path / "umi_bins.tsv").readline() == "#bin\tumi\treads\tdistinct\tlength\n"
    summary = {r["status"]: r["reads"] for r in umi.read_table(str(tmp_path / "umi_summary.tsv"))}
    assert summary == dict(ok=int((run["molecule"] >= 0).sum()), no_umi=3, bad_len=3, small_bin=0)
    from ngspeciesid_amd import classify
    lib = classify.read_reference_fasta(str(tmp_path / "umi_consensus.fasta"), unique_names=False)
    assert [lib.rs.get(i)[0] for i in range(lib.rs.n)] == res["polished"]
    assert lib.headers == ["umi_%d;reads=%d;umi=%s" % (b, int(bn["reads"][b]), bn["umis"][bn["centroids"][b]]) for b in res["kept"]]
