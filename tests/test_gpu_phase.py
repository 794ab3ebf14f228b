"""GPU: the three calls of include/ngsid_phase.h through the C-ABI == their definition restated from the oracle's parts (tests/phase_reference.py), code for code and
integer for integer, and the pipeline / CLI layers on top of them."""
import os
import numpy as np
import pytest
from ngspeciesid_amd import synth, pipeline
from ngspeciesid_amd._capi import ReadSet, NgsidError, phase_offsets
from phase_reference import PhaseAdapter, genotypes_reference, pair_tables_numpy, assign_numpy
import phase_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def groups():
    """3 groups of 200, 64 and 1 reads, centres of 400 / 330 / 300 bases (the first with a homopolymer of 7 at 120), mu = 14, both strands; three reads with N, one random read"""
    sp = [synth.make_species(1, L, 0.0, indel=0.0, seed=90 + L)[0].tobytes().decode() for L in (400, 330, 300)]
    sp[0] = pc.with_homopolymers(sp[0], [(120, 7)])
    sets = [pc.reads_of(sp[g], n, 14.0, 91 + g) for g, n in enumerate((200, 64, 1))]
    reads = [s.get(i)[0] for s in sets for i in range(s.n)]
    for i, p in ((5, 0), (17, 122), (210, 100)):                                     # runs of 8 N: mismatches with a base outside ACGT, whatever the strand
        reads[i] = reads[i][:p] + "N" * 8 + reads[i][p + 8:]
    rng = np.random.default_rng(3)
    reads[40] = "".join("ACGT"[int(v)] for v in rng.integers(4, size=380))          # shares no minimizer with its centre: strand -1
    return sp, ReadSet.from_strings(reads), np.array([0, 200, 264, 265], dtype=np.uint64)


SITE_LISTS = {
    "ends_adjacent_homopolymer": [[0, 122, 123, 399], [100, 101], [150]],          # position 0 with the last one, inside the homopolymer, two adjacent positions
    "64_and_empty": [np.unique(np.linspace(0, 399, 64).astype(int)).tolist(), [], [0, 299]],
}


def _sites(lists):
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
    return off, np.array([p for x in lists for p in x], dtype=np.uint32)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", sorted(SITE_LISTS))
def test_genotypes_equal_the_reference(gpu_api, oracle, groups, name, clip):
    centres, rs, grp = groups
    site_off, site_pos = _sites(SITE_LISTS[name])
    if name == "64_and_empty": assert site_off[1] == 64
    got = gpu_api.phase_genotypes(ReadSet.from_strings(centres), rs, grp, site_off, site_pos, clip=clip)
    exp = genotypes_reference(oracle, centres, rs, grp, site_off, site_pos, None, 13, 20, clip)
    assert np.array_equal(got[2], exp[2]) and got[2][40] == -1 and (got[2] == 1).sum() > 50
    assert np.array_equal(got[1], exp[1])
    bad = np.nonzero(got[0] != exp[0])[0]
    assert len(bad) == 0, "%d codes differ, first at %d: HIP %d reference %d" % (len(bad), bad[0], got[0][bad[0]], exp[0][bad[0]])
    g0 = got[0][:int(got[1][1])].reshape(200, -1)
    assert (g0[40] == 7).all() and set(np.unique(got[0]).tolist()) <= {0, 1, 2, 3, 4, 5, 7}
    if name == "64_and_empty":
        assert (g0[17] == 5).any() and (got[0] == 4).any() and (g0 <= 3).mean() > 0.8      # a site every 6 bases meets the run of N; deletions occur; most codes are bases
    else:
        sup = gpu_api.consensus_support(ReadSet.from_strings(centres), rs, grp, clip=clip)[0]
        for j, p in enumerate(SITE_LISTS[name][0]):                                   # the invariant against the support call of the same library
            h = np.bincount(g0[:, j], minlength=8)
            assert h[:6].sum() == sup[p, 0] and h[4] == sup[p, 6] and h[:4].sum() == sup[p, 1:6].sum()


def test_genotypes_in_chunks_and_unbanded(gpu_api):
    """the same call with a path matrix of 1 MB at a time and with the unbanded instances: same codes.  6 000 reads of 300 - 600 bases: more than one chunk, and the
    length-class launches of a large batch"""
    sp = synth.make_species(3, 500, 0.15, seed=64)
    rd = synth.make_reads(sp, 6000, mu=14.0, seed=65, rc_fraction=0.5)
    rs = ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64)); species = rd["species"].numpy()
    lists = [np.nonzero(species == g)[0].astype(np.uint32) for g in range(3)]
    grp = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64); ro = np.concatenate(lists)
    centres = [s.tobytes().decode() for s in sp]
    site_off, site_pos = _sites([np.unique(np.linspace(0, len(c) - 1, 64).astype(int)).tolist() for c in centres])
    cen = ReadSet.from_strings(centres)
    base = gpu_api.phase_genotypes(cen, rs, grp, site_off, site_pos, read_order=ro)
    assert (base[0] <= 3).mean() > 0.8
    for opt, val in (("support_budget_mb", 1), ("ed_band", 0)):
        gpu_api.set_option(opt, val)
        try:
            again = gpu_api.phase_genotypes(cen, rs, grp, site_off, site_pos, read_order=ro)
        finally:
            gpu_api.set_option(opt, 0 if opt == "support_budget_mb" else -1)
        assert all(np.array_equal(x, y) for x, y in zip(base, again)), opt


def test_genotype_argument_errors(gpu_api, groups):
    centres, rs, grp = groups
    cen = ReadSet.from_strings(centres)
    for lists in ([list(range(65)), [], []], [[10, 5], [], []], [[10, 10], [], []], [[], [330], []], [[], [], [0, 300]]):
        site_off, site_pos = _sites(lists)
        with pytest.raises(NgsidError) as ex:
            gpu_api.phase_genotypes(cen, rs, grp, site_off, site_pos)
        assert ex.value.code == -2
    ok = gpu_api.phase_genotypes(cen, rs, grp, *_sites([[], [329], [299]]))
    assert len(ok[0]) == 65


def _random_geno(rng, R, S, p_none=0.05):
    g = rng.choice(np.array([0, 1, 2, 3, 4, 5, 7], dtype=np.uint8), size=(R, S), p=[0.55, 0.2, 0.05, 0.05, 0.05, 0.05 - p_none / 2, 0.05 + p_none / 2])
    return g


def test_pair_tables_equal_numpy(gpu_api, groups):
    """S = 1 (all zero), 2 and 64; R = 1, 1 025 and 4 097 (one more than a slice of k_phase_pairs); a group whose reads all have code 7; an empty group; and the
    genotypes the library itself returns for the read groups of this file"""
    rng = np.random.default_rng(11)
    shapes = [(1025, 64), (1, 2), (300, 1), (50, 2), (4097, 3), (0, 5), (130, 64)]
    blocks = [_random_geno(rng, R, S) for R, S in shapes]
    blocks[3][:] = 7
    grp = np.concatenate(([0], np.cumsum([R for R, _ in shapes]))).astype(np.uint64); site_off = np.concatenate(([0], np.cumsum([S for _, S in shapes]))).astype(np.uint64)
    geno = np.concatenate([b.ravel() for b in blocks])
    got, toff = gpu_api.phase_pair_tables(geno, grp, site_off)
    exp, eoff = pair_tables_numpy(geno, grp, site_off)
    assert np.array_equal(toff, eoff) and np.array_equal(got, exp)
    for g, (R, S) in enumerate(shapes):
        t = got[int(toff[g]):int(toff[g + 1])].reshape(S, S, 5, 5)
        assert t[np.tril_indices(S)].sum() == 0
        cover = (blocks[g] <= 4).sum(axis=0)
        for s in range(S):
            for u in range(s + 1, S):
                assert t[s, u].sum(axis=1).sum() <= min(cover[s], cover[u]) and (t[s, u].sum(axis=1) <= np.bincount(blocks[g][:, s], minlength=8)[:5]).all() \
                    and (t[s, u].sum(axis=0) <= np.bincount(blocks[g][:, u], minlength=8)[:5]).all()
    assert got[int(toff[2]):int(toff[3])].sum() == 0 and got[int(toff[3]):int(toff[4])].sum() == 0 and got[:int(toff[1])].sum() > 1025 * 1000
    centres, rs, rgrp = groups
    so, sp_ = _sites(SITE_LISTS["64_and_empty"])
    g2 = gpu_api.phase_genotypes(ReadSet.from_strings(centres), rs, rgrp, so, sp_)[0]
    a, b = gpu_api.phase_pair_tables(g2, rgrp, so), pair_tables_numpy(g2, rgrp, so)
    assert np.array_equal(a[0], b[0]) and a[0].sum() > 0


def test_assign_equals_numpy(gpu_api):
    """H = 1, 2, 16 and 0, wildcards, ties (lowest haplotype, dist2 == dist), reads without a covered site, more reads than a workgroup"""
    rng = np.random.default_rng(12)
    shapes = [(700, 64, 16), (300, 5, 2), (40, 3, 1), (20, 4, 0), (10, 0, 0), (257, 2, 2)]
    blocks = [_random_geno(rng, R, S, p_none=0.1) for R, S, _ in shapes]
    blocks[1][:7] = 7; blocks[1][7:12] = 5                                            # all-uncovered reads
    haps = []
    for (R, S, H), b in zip(shapes, blocks):
        h = rng.integers(0, 5, size=(H, S)).astype(np.uint8)
        h[rng.random((H, S)) < 0.2] = 255
        haps.append(h)
    haps[0][1] = 0; haps[0][3] = haps[0][1]                                           # the major allele everywhere, twice: every read nearest to it is tied: every read nearest to them is tied
    haps[5][:] = [[0, 1], [0, 1]]
    grp = np.concatenate(([0], np.cumsum([s[0] for s in shapes]))).astype(np.uint64); site_off = np.concatenate(([0], np.cumsum([s[1] for s in shapes]))).astype(np.uint64)
    hap_off = np.concatenate(([0], np.cumsum([s[2] for s in shapes]))).astype(np.uint64)
    geno = np.concatenate([b.ravel() for b in blocks]); hal = np.concatenate([h.ravel() for h in haps])
    got = gpu_api.phase_assign(geno, grp, site_off, hap_off, hal)
    exp = assign_numpy(geno, grp, site_off, hap_off, hal)
    for x, y, what in zip(got, exp, ("best", "dist", "dist2")):
        assert np.array_equal(x, y), what
    best, dist, dist2 = got
    a = int(grp[1])
    assert (best[a:a + 12] == -1).all() and (dist[a:a + 12] == 255).all() and (dist2[a:a + 12] == 255).all()
    assert (best[int(grp[3]):int(grp[5])] == -1).all() and (dist2[int(grp[2]):int(grp[3])] == 255).all() and (best[int(grp[2]):int(grp[3])] <= 0).all()
    tied = best[:700] == 1
    assert tied.any() and not (best[:700] == 3).any() and (dist2[:700][tied] == dist[:700][tied]).all()
    last = slice(int(grp[5]), int(grp[6])); cov = best[last] >= 0
    assert cov.sum() > 200 and (best[last][cov] == 0).all() and (dist2[last][cov] == dist[last][cov]).all()
    with pytest.raises(NgsidError):
        gpu_api.phase_assign(np.zeros(17, np.uint8), [0, 1], [0, 17], [0, 17], np.zeros(17 * 17, np.uint8))


@pytest.fixture(scope="module")
def three(oracle):
    T = pc.three_templates()
    rs, origin = pc.pooled(T, 150, 17.0, pc.SPLIT_SEED)
    sub, score, org = pc.score_ordered(oracle, rs, origin)
    return T, rs, sub, score, dict(pc.KW, acc_rank=np.arange(sub.n, dtype=np.uint32))


def _same_haplotypes(xs, ys):
    assert [e is None for e in xs] == [e is None for e in ys]
    for x, y in zip(xs, ys):
        if x is None: continue
        assert sorted(x) == sorted(y)
        for key in x:
            if isinstance(x[key], np.ndarray): assert np.array_equal(x[key], y[key]) and x[key].dtype == y[key].dtype, key
            else: assert x[key] == y[key], key


def test_pipeline_through_hip_equals_the_adapter(gpu_api, oracle, three):
    T, _, sub, score, kw = three
    a = pipeline.run_hot_path(gpu_api, sub, score, split_haplotypes=True, **kw)
    b = pipeline.run_hot_path(PhaseAdapter(oracle), sub, score, split_haplotypes=True, **kw)
    assert a["centers"] == b["centers"] and len(a["haplotypes"]) == len(b["haplotypes"]) == 2
    assert [e is None for e in a["haplotypes"]] == [e is None for e in b["haplotypes"]] and sum(e is not None for e in a["haplotypes"]) == 1
    _same_haplotypes(a["haplotypes"], b["haplotypes"])
    # the same from a device-resident (torch-backed) read set, as bench.py hands the reads over
    import torch
    dev = ReadSet.from_torch(torch.from_numpy(sub.seq).cuda(), torch.from_numpy(sub.qual).cuda(), torch.from_numpy(sub.off.astype(np.int64)).cuda())
    c = pipeline.run_hot_path(gpu_api, dev, score, split_haplotypes=True, **kw)
    assert c["centers"] == a["centers"]
    _same_haplotypes(c["haplotypes"], a["haplotypes"])
    plain = pipeline.run_hot_path(gpu_api, sub, score, **kw)
    assert sorted(plain) == sorted(k for k in a if k != "haplotypes") and plain["centers"] == a["centers"] and np.array_equal(plain["rep_of"], a["rep_of"])


def _files(out):
    res = {}
    for root, _, fs in os.walk(out):
        for f in fs:
            res[os.path.relpath(os.path.join(root, f), out)] = open(os.path.join(root, f), "rb").read()
    return res


def test_cli_flag(gpu_api, tmp_path, three):
    from ngspeciesid_amd import cli as _cli, fastpath
    T, rs, _, _, _ = three
    fq = str(tmp_path / "in.fastq")
    with open(fq, "w") as f:
        for i in range(rs.n):
            s, q = rs.get(i)
            f.write("@r%d\n%s\n+\n%s\n" % (i, s, q))
    res = []
    for flag in ([], ["--split_haplotypes"]):
        out = str(tmp_path / ("o%d" % len(flag))); os.makedirs(out)
        args = _cli.build_parser().parse_args(["--ont", "--fastq", fq, "--outfolder", out, "--t", "1", "--consensus", "--racon", "--racon_iter", "2", "--abundance_ratio", "0.05"] + flag); args.k, args.w = 13, 20
        fastpath.main(args, api=gpu_api)
        res.append(_files(out))
    a, b = res
    assert set(a) <= set(b) and all(a[f] == b[f] for f in a if f != "logfile.txt")
    new = sorted(set(b) - set(a))
    rows = b["haplotypes.tsv"].decode().splitlines()
    assert rows[0].split("\t") == ["cluster_id", "haplotype", "reads", "sites", "alleles"] and len(rows) == 3
    cid = rows[1].split("\t")[0]
    assert [r.split("\t")[:2] for r in rows[1:]] == [[cid, "0"], [cid, "1"]]
    fas = [os.path.join("racon_cl_id_" + cid, "consensus_h%d.fasta" % j) for j in (0, 1)]
    assert new == sorted(["haplotypes.tsv"] + fas)
    rc = pipeline.revcomp_str; found = set()
    for j, fa in enumerate(fas):
        head, seq = b[fa].decode().split("\n")[:2]
        n = int(rows[1 + j].split("\t")[2])
        assert head.startswith(">consensus_cl_id_%s_h%d_total_supporting_reads_%d LN:i:%d RC:i:" % (cid, j, n, len(seq))) and 100 < n <= 150
        assert len(rows[1 + j].split("\t")[3].split(",")) == len(rows[1 + j].split("\t")[4]) == 3
        found.add(next((t for t in (0, 1) if seq in (T[t], rc(T[t]))), None))
    assert found == {0, 1}
    # with --reference_db the haplotypes are rows of classification.tsv under their ids, behind the clusters' own rows, each naming its own template
    lib = str(tmp_path / "lib.fasta")
    with open(lib, "w") as f:
        for t in range(3): f.write(">tmpl%d\n%s\n" % (t, T[t]))
    out = str(tmp_path / "o_db"); os.makedirs(out)
    args = _cli.build_parser().parse_args(["--ont", "--fastq", fq, "--outfolder", out, "--t", "1", "--consensus", "--racon", "--racon_iter", "2", "--abundance_ratio", "0.05", "--split_haplotypes",
                                           "--reference_db", lib, "--classify_report", "1"]); args.k, args.w = 13, 20
    fastpath.main(args, api=gpu_api)
    c = _files(out)
    assert c["haplotypes.tsv"] == b["haplotypes.tsv"] and all(c[fa] == b[fa] for fa in fas)
    tab = [r.split("\t") for r in c["classification.tsv"].decode().splitlines()[1:]]
    ids = [r[0] for r in tab]
    assert len(ids) == 4 and ["_h" in i for i in ids] == [False, False, True, True] and ids[2].startswith("consensus_cl_id_%s_h0_" % cid) and ids[3].startswith("consensus_cl_id_%s_h1_" % cid)
    named = {r[0]: r[3] for r in tab}
    assert {named[ids[2]], named[ids[3]]} == {"tmpl0", "tmpl1"}
