"""GPU: ngsid_umi_pairs (include/ngsid_umi.h, csrc/k_umi.hip) through Api.umi_pairs against the brute force of tests/umi_reference.py - pairs, order and distances, every
comparison exact - and the UMI mode (ngspeciesid_amd/umi.py) end to end on reads of 24 molecules, through umi.run and through the command line."""
import functools
import os
import numpy as np
import pytest
import variants_cases as vc
import umi_reference as ur
import umi_cases as uc
from ngspeciesid_amd import umi
from ngspeciesid_amd._capi import ReadSet, NgsidError

pytestmark = pytest.mark.gpu
DESIGN = umi.Design(*uc.FLANKS, umi_len=uc.UMI_LEN, len_slack=uc.LEN_SLACK)


def _triples(got):
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and got[2].dtype == np.uint8
    return list(zip(got[0].tolist(), got[1].tolist(), got[2].tolist()))


def _check(api, seqs, d, g, what):
    want = ur.pairs(seqs, d)
    got = _triples(api.umi_pairs(seqs, d, g))
    assert len(got) == len(set((i, j) for i, j, _ in got)), "%s: a pair was emitted twice" % what
    assert got == want, "%s: %d pairs, want %d; first difference %s" % (what, len(got), len(want), next(((a, b) for a, b in zip(got, want) if a != b), None))
    return got


@functools.lru_cache(maxsize=None)
def _set(d, g):
    return uc.search_set(np.random.default_rng(1000 * d + g), d, g)


@pytest.mark.parametrize("g", (4, 9, 16))
@pytest.mark.parametrize("d", (0, 1, 3, 8))
def test_search_set_against_brute_force(gpu_api, d, g):
    """the border lengths, the only-intact-seed pairs at shifts +d and -d, substrings at the edges, exactly d and d + 1, N in seeds, the dedupe families; at
    seed_len 16 with max_dist 8 (and wherever (d + 1) g exceeds 64) everything goes down the short path"""
    seqs = _set(d, g)
    got = _check(gpu_api, seqs, d, g, "d=%d g=%d" % (d, g))
    assert len(got) >= 20 and {0, d} <= {x[2] for x in got}


def test_identical_sequences_one_large_bucket(gpu_api):
    seqs = [vc.rand_seq(np.random.default_rng(2), 36)] * 300
    pi, pj, dist = gpu_api.umi_pairs(seqs, 3, 9)
    assert len(pi) == 44850 and not dist.any()
    assert list(zip(pi.tolist(), pj.tolist())) == [(i, j) for i in range(300) for j in range(i + 1, 300)]


def test_tiny_sets(gpu_api):
    for seqs in ([], ["ACGT"], [""], ["ACGT", "ACGA"], ["", ""], ["", "A"], ["ACGT" * 9, "ACGT" * 9]):
        for d, g in ((0, 4), (1, 4), (3, 9)):
            _check(gpu_api, seqs, d, g, "%r d=%d" % (seqs, d))


@functools.lru_cache(maxsize=None)
def _families():
    seqs, _ = vc.families(np.random.default_rng(21), 50, 20, 36, 0.05)
    return [s[:64] for s in seqs]


def test_equals_near_pairs_on_a_family_set(gpu_api):
    seqs = _families()
    assert len(seqs) == 1000
    a = gpu_api.near_pairs(seqs, 3, both_strands=False)
    b = gpu_api.umi_pairs(seqs, 3, 9)
    assert len(b[0]) > 2000
    for x, y in zip(a[:3], b): assert x.dtype == y.dtype and np.array_equal(x, y)


def test_chunking_and_permutation_do_not_change_the_result(gpu_api):
    seqs = _families()[:400] + _set(3, 4)[:60]
    want = _check(gpu_api, seqs, 3, 8, "default chunks")
    try:
        for chunk in (1, 64, 65):
            gpu_api.set_option("umi_chunk_seqs", chunk)
            assert _triples(gpu_api.umi_pairs(seqs, 3, 8)) == want, chunk
    finally:
        gpu_api.set_option("umi_chunk_seqs", 0)
    perm = np.random.default_rng(4).permutation(len(seqs))
    pi, pj, dist = gpu_api.umi_pairs([seqs[p] for p in perm], 3, 8)
    back = sorted((min(int(perm[i]), int(perm[j])), max(int(perm[i]), int(perm[j])), int(d)) for i, j, d in zip(pi, pj, dist))
    assert back == want
    for g in (4, 6, 12, 16):
        assert _triples(gpu_api.umi_pairs(seqs, 3, g)) == want, g


@pytest.mark.parametrize("max_tiles", [1, 7, 64])
def test_the_tile_cap_of_a_join_chunk_does_not_change_the_result(gpu_api, max_tiles):
    """umi_max_tiles lowers the tiles one join chunk takes: the queries are split as they are beyond the real bound of a launch (tests/test_gpu_launch_bound.py), a
    query of more tiles than the cap still goes in one launch"""
    seqs = _families()
    want = _triples(gpu_api.umi_pairs(seqs, 3, 9))
    assert len(want) > 2000
    try:
        gpu_api.set_option("umi_max_tiles", max_tiles)
        assert _triples(gpu_api.umi_pairs(seqs, 3, 9)) == want
    finally:
        gpu_api.set_option("umi_max_tiles", 0)
        gpu_api.set_option("release_scratch", 1)


def test_cap_protocol(gpu_api):
    seqs = _families()[:200]
    want = _triples(gpu_api.umi_pairs(seqs, 3, 9))
    n = len(want)
    assert n > 10
    assert _triples(gpu_api.umi_pairs(seqs, 3, 9, cap=n)) == want and _triples(gpu_api.umi_pairs(seqs, 3, 9, cap=n + 100)) == want
    for cap in (n - 1, 1):
        with pytest.raises(NgsidError) as e:
            gpu_api.umi_pairs(seqs, 3, 9, cap=cap)
        assert e.value.code == -4 and e.value.needed == n


def test_errors(gpu_api):
    ok = ["ACGT" * 9, "ACGT" * 9]
    for seqs, d, g, code in ((["A" * 65, "ACGT"], 3, 9, -6), (["ACGt", "ACGT"], 3, 9, -3), (ok, 9, 9, -2), (ok, -1, 9, -2), (ok, 3, 3, -2), (ok, 3, 17, -2)):
        with pytest.raises(NgsidError) as e:
            gpu_api.umi_pairs(seqs, d, g)
        assert e.value.code == code, (seqs, d, g)
    assert len(gpu_api.umi_pairs(["A" * 64, "A" * 64], 8, 16)[0]) == 1


def test_profile_lines(gpu_api):
    gpu_api.profile_enable(True)
    try:
        gpu_api.profile_read()
        gpu_api.umi_pairs(_set(3, 4), 3, 4)
        tot, _ = gpu_api.profile_read()
    finally:
        gpu_api.profile_enable(False)
    assert {"k_umi_keys", "k_umi_sort", "k_umi_join", "k_umi_short", "umi_candidates"} <= set(tot) and tot["umi_candidates"][0] > 0


@functools.lru_cache(maxsize=None)
def _run():
    return uc.make_run(5)


def test_end_to_end_bins_and_consensus(gpu_api, tmp_path):
    """3 templates x 8 molecules x 6 reads: the bins equal the reference's read for read, every bin's draft and polished sequence are what Api.poa_consensus and
    Api.polish return for the same groups called directly, and every polished sequence equals its template (as on the CPU oracle: tests/test_umi_cpu.py)"""
    from ngspeciesid_amd.pipeline import group_offsets
    run = _run()
    rs = ReadSet.from_strings(run["seqs"], run["quals"])
    res = umi.run(gpu_api, rs, DESIGN, window=150, flank_max_ed=3, max_dist=3, min_reads=3, racon_iter=3)
    ex = ur.extract(run["seqs"], uc.FLANKS, uc.UMI_LEN, uc.LEN_SLACK, 150, 3)
    assert res["extract"]["key"] == [e[2] for e in ex]
    rbin, rows, small = ur.bins([e[2] for e in ex], 3, 3)
    assert res["bin"].tolist() == rbin and res["bins"]["small"].tolist() == small
    assert len(res["kept"]) == len(run["umis"]) == 24
    work = umi.trimmed_oriented(rs, res["extract"])
    lists = [np.flatnonzero(np.array(rbin) == b).astype(np.uint32) for b in res["kept"]]
    assert all(np.array_equal(a, b) for a, b in zip(lists, res["lists"]))
    draft_prm, polish_prm = umi.consensus_params(3)
    drafts = list(gpu_api.poa_consensus(work, group_offsets(lists), draft_prm, read_order=np.concatenate(lists)))
    polished = list(gpu_api.polish(ReadSet.from_strings(drafts), work, group_offsets(lists), polish_prm, read_order=np.concatenate(lists))[0])
    assert res["drafts"] == drafts and res["polished"] == polished
    for b, seq in zip(res["kept"], res["polished"]):
        mol = {int(run["molecule"][r]) for r in lists[res["kept"].index(b)]}
        assert len(mol) == 1 and seq == run["templates"][run["template_of"][mol.pop()]], b
    # the sub-command writes the same four files
    import demux_reference as dr
    from ngspeciesid_amd.cli import cli
    fq = tmp_path / "reads.fastq"
    dr.write_fastq(str(fq), run["names"], run["seqs"], run["quals"])
    (tmp_path / "a").mkdir()
    umi.write(str(tmp_path / "a"), run["names"], res)
    with pytest.raises(SystemExit) as e:
        cli(["umi", "--fastq", str(fq), "--outfolder", str(tmp_path / "b"), "--umi_fwd", ",".join(uc.FLANKS[:2]), "--umi_rev", ",".join(uc.FLANKS[2:])])
    assert e.value.code == 0
    for f in ("umi_consensus.fasta", "umi_bins.tsv", "umi_reads.tsv", "umi_summary.tsv"):
        assert open(tmp_path / "a" / f).read() == open(tmp_path / "b" / f).read(), f
    assert open(tmp_path / "b" / "umi_consensus.fasta").read().count(">") == 24
