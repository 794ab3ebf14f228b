"""CPU: the policy of ngspeciesid_amd/phase.py on hand-made inputs, the reference definition of the device calls (tests/phase_reference.py) against the support
reference, and the pipeline's split through the oracle-backed adapter (the oracle has no twin of the phase calls: the HIP library is checked against the same definition in
tests/test_gpu_phase.py)."""
import numpy as np
import pytest
from ngspeciesid_amd import phase, pipeline, cli
from ngspeciesid_amd._capi import ReadSet
from support_reference import support_reference
from phase_reference import PhaseAdapter, genotypes_reference, pair_tables_numpy, assign_numpy
import phase_cases as pc


def _counts(rows):
    """[len, 8] counters from (depth, agree, A, C, G, T, del) rows"""
    c = np.zeros((len(rows), 8), dtype=np.uint32); c[:, :7] = rows
    return c


def test_candidate_sites_at_the_bound():
    # centre AAAA, depth 100: the second allele (C) at 15 = ceil(0.15 * 100) is a site, at 14 it is not; depth 20: the bound is min_alt_reads = 5, 5 is a site and 4 is not;
    # a deletion counts as an allele; a base whose ONLY allele is a substitution (no agree) has a second count of 0
    c = _counts([(100, 85, 0, 15, 0, 0, 0), (100, 86, 0, 14, 0, 0, 0), (20, 15, 0, 0, 5, 0, 0), (20, 16, 0, 0, 4, 0, 0), (100, 80, 0, 0, 0, 0, 20), (100, 0, 0, 100, 0, 0, 0)])
    assert phase.candidate_sites(c, "AAAAAA", 0.15, 5).tolist() == [0, 2, 4]
    # the centre's own base takes `agree`: centre C with 40 reads of A against 60 agreeing ones is a site whose second count is 40
    assert phase.candidate_sites(_counts([(100, 60, 40, 0, 0, 0, 0)]), "C", 0.15, 5).tolist() == [0]
    assert phase.allele_counts(_counts([(100, 60, 40, 0, 0, 0, 0)]), "C").tolist() == [[40, 60, 0, 0, 0]]


def test_candidate_sites_more_than_64():
    # 70 candidates: positions 0 - 59 with a second count of 30, 60 - 69 with 40 -> the ten strong ones and the FIRST 54 of the equal ones, ascending
    rows = [(100, 70, 0, 30, 0, 0, 0)] * 60 + [(100, 60, 0, 40, 0, 0, 0)] * 10
    got = phase.candidate_sites(_counts(rows), "A" * 70, 0.15, 5)
    assert got.tolist() == list(range(54)) + list(range(60, 70)) and got.dtype == np.uint32
    assert phase.candidate_sites(_counts(rows), "A" * 70, 0.15, 5, max_sites=3).tolist() == [60, 61, 62]


def _table(pairs):
    t = np.zeros((5, 5), dtype=np.uint32)
    for (a, b), n in pairs.items(): t[a, b] = n
    return t


def test_linked_sites_phi():
    # sites 0 and 1: A/A 50, C/G 50 -> phi = 1.  Site 2 is independent of both (every cell 25): phi = 0.  Site 2's own alleles: A 50 / G 50, two bases at 50 % -> kept as a
    # single.  Site 3: independent, alleles A 80 / del 20 -> a lone del site is dropped.  Site 4: independent, A 90 / C 10 -> minor fraction 0.1 < 0.25, dropped.
    S = 5; t = np.zeros((S, S, 5, 5), dtype=np.uint32)
    t[0, 1] = _table({(0, 0): 50, (1, 2): 50})
    t[0, 2] = _table({(0, 0): 25, (0, 2): 25, (1, 0): 25, (1, 2): 25}); t[1, 2] = _table({(0, 0): 25, (0, 2): 25, (2, 0): 25, (2, 2): 25})
    for s, (a, b) in ((0, (0, 1)), (1, (0, 2)), (2, (0, 2))):
        t[s, 3] = _table({(a, 0): 40, (a, 4): 10, (b, 0): 40, (b, 4): 10}); t[s, 4] = _table({(a, 0): 45, (a, 1): 5, (b, 0): 45, (b, 1): 5})
    t[3, 4] = _table({(0, 0): 72, (0, 1): 8, (4, 0): 18, (4, 1): 2})
    assert phase.pair_phi(t[0, 1]) == pytest.approx(1.0) and phase.pair_phi(t[0, 2]) == 0.0 and phase.pair_phi(t[3, 4]) == pytest.approx(0.0)
    sc = np.array([[50, 50, 0, 0, 0], [50, 0, 50, 0, 0], [50, 0, 50, 0, 0], [80, 0, 0, 0, 20], [90, 10, 0, 0, 0]])
    assert phase.linked_sites(t, 0.5, 0.25, site_counts=sc).tolist() == [True, True, True, False, False]
    assert phase.linked_sites(t, 0.5, 0.25).tolist() == [True, True, True, False, False]          # the same from the tables' own marginals
    # the top-two reduction takes the lower code on ties: A 40 / C 40 / G 40 reduces to A and C
    assert phase._top2([40, 40, 40, 0, 0]) == (0, 1)
    # a single site: no table at all
    assert phase.linked_sites(np.zeros((1, 1, 5, 5)), 0.5, 0.25, site_counts=[[60, 0, 0, 40, 0]]).tolist() == [True]
    assert phase.linked_sites(np.zeros((1, 1, 5, 5)), 0.5, 0.25, site_counts=[[60, 0, 0, 0, 40]]).tolist() == [False]


def test_haplotype_order_and_bounds():
    # strings over sites (0, 2) [site 1 is not kept]: "AC" x 12, "CA" x 12, "AA" x 10, "GG" x 9, one read with an uncovered kept site, one with code 5
    rows = [(0, 7, 1)] * 12 + [(1, 7, 0)] * 12 + [(0, 3, 0)] * 10 + [(2, 0, 2)] * 9 + [(0, 0, 7), (5, 0, 1)]
    g = np.array(rows, dtype=np.uint8)
    al, cnt = phase.haplotypes(g, [0, 2], min_hap_reads=10, min_hap_frac=0.05)
    assert al.tolist() == [[0, 1], [1, 0], [0, 0]] and cnt.tolist() == [12, 12, 10]          # ties in count: the lexicographically smaller string first; 9 < 10 is out
    assert phase.haplotypes(g, np.array([True, False, True]), 10, 0.05, max_haps=2)[0].tolist() == [[0, 1], [1, 0]]
    assert phase.haplotypes(g, [0, 2], min_hap_reads=1, min_hap_frac=0.25)[1].tolist() == [12, 12]      # ceil(0.25 * 43) = 11
    assert phase.haplotypes(g, [0, 2], min_hap_reads=12, min_hap_frac=0.0)[1].tolist() == [12, 12]
    assert phase.haplotypes(g, [0, 2], min_hap_reads=13, min_hap_frac=0.0) is None and phase.haplotypes(g, [], 1, 0.0) is None
    # allowed: strings over the two named alleles of each site only ("GG" goes, although 9 reads carry it); the bound still counts all 43 fully covered reads
    assert phase.haplotypes(g, [0, 2], 9, 0.0)[1].tolist() == [12, 12, 10, 9]
    assert phase.haplotypes(g, [0, 2], 9, 0.0, allowed=[(0, 1), (0, 1)])[0].tolist() == [[0, 1], [1, 0], [0, 0]]
    assert phase.haplotypes(g, [0, 2], 1, 0.25, allowed=[(0, 1), (0, 1)])[1].tolist() == [12, 12]
    assert phase.haplotypes(g, [0, 2], 1, 0.0, allowed=[(3, 4), (3, 4)]) is None


def test_margin_rule():
    best = np.array([0, 1, 0, -1, 1], dtype=np.int8); dist = np.array([0, 1, 1, 255, 0], dtype=np.uint8); dist2 = np.array([1, 1, 3, 255, 255], dtype=np.uint8)
    assert phase.apply_margin(best, dist, dist2, 1).tolist() == [0, -1, 0, -1, 1]
    assert phase.apply_margin(best, dist, dist2, 2).tolist() == [-1, -1, 0, -1, 1]


def test_assign_and_tables_numpy_hand_values():
    geno = np.array([[0, 1], [0, 1], [2, 3], [7, 3], [5, 4]], dtype=np.uint8).ravel()
    tab, off = pair_tables_numpy(geno, [0, 5], [0, 2])
    t = tab.reshape(2, 2, 5, 5)
    assert off.tolist() == [0, 100] and t[0, 1, 0, 1] == 2 and t[0, 1, 2, 3] == 1 and t.sum() == 3
    best, d, d2 = assign_numpy(geno, [0, 5], [0, 2], [0, 2], np.array([[0, 1], [2, 255]], dtype=np.uint8))
    # read 3 covers site 1 only (code 3): h0 differs there, h1 has a wildcard; read 4 has code 5 at site 0 (not compared) and a deletion at site 1
    assert best.tolist() == [0, 0, 1, 1, 1] and d.tolist() == [0, 0, 0, 0, 0] and d2.tolist() == [1, 1, 2, 1, 1]
    best, d, d2 = assign_numpy(np.array([7, 5, 0, 0], dtype=np.uint8), [0, 2], [0, 2], [0, 1], np.array([[1, 1]], dtype=np.uint8))
    assert best.tolist() == [-1, 0] and d.tolist() == [255, 2] and d2.tolist() == [255, 255]


def test_reference_genotypes_equal_the_support_counters(oracle):
    """per site, the histogram of the reference's genotype codes is the support reference's row: depth = codes <= 5, agree = the centre's base, sub_*, del"""
    T = pc.three_templates()
    centre = pc.with_homopolymers(T[0], [(150, 6)])
    rs, _ = pc.pooled([centre, pc.variant(centre, (40, 300))], [60, 40], 14.0, 31)
    reads = [rs.get(i)[0] for i in range(rs.n)]
    reads[3] = reads[3][:50] + "N" + reads[3][51:]; reads[7] = "AG" * 150
    rs = ReadSet.from_strings(reads); grp = np.array([0, rs.n], dtype=np.uint64)
    for clip in (False, True):
        counts, _, used, strand = support_reference(oracle, [centre], rs, grp, None, 13, 20, clip)
        sites = np.arange(len(centre), dtype=np.uint32)[::7][:64]
        geno, goff, st = genotypes_reference(oracle, [centre], rs, grp, [0, len(sites)], sites, None, 13, 20, clip)
        assert np.array_equal(st, strand) and st[7] == -1 and goff.tolist() == [0, rs.n * len(sites)]
        g = geno.reshape(rs.n, len(sites)); cb = ["ACGT".index(centre[int(p)]) for p in sites]
        assert (g[7] == 7).all()
        for j, p in enumerate(sites):
            h = np.bincount(g[:, j], minlength=8); row = counts[int(p)]
            exp_alleles = [int(row[2 + c]) + (int(row[1]) if c == cb[j] else 0) for c in range(4)]
            assert h[:6].sum() == row[0] and h[:4].tolist() == exp_alleles and h[4] == row[6] and h[6] == 0, (clip, int(p))
        assert int(used[0]) == int((g != 7).any(axis=1).sum()) or len(sites) < len(centre)


# Seeds tried for the read set below (the `seed` of pc.pooled): 500, 600 and 700 - each splits into the two templates with no read misplaced, and the margin rule leaves
# out 0, 0.34 % and 0.34 % of the cluster's reads (the reference, through this file's adapter).  500 is the one kept.
SPLIT_SEED = pc.SPLIT_SEED


@pytest.fixture(scope="module")
def three(oracle):
    T = pc.three_templates()
    rs, origin = pc.pooled(T, 150, 17.0, SPLIT_SEED)
    sub, score, org = pc.score_ordered(oracle, rs, origin)
    kw = dict(pc.KW, acc_rank=np.arange(sub.n, dtype=np.uint32))
    return T, sub, score, org, kw


def test_split_through_the_adapter(oracle, three):
    T, sub, score, origin, kw = three
    res = pipeline.run_hot_path(PhaseAdapter(oracle), sub, score, split_haplotypes=True, **kw)
    haps = res["haplotypes"]
    assert len(haps) == len(res["centers"]) == 2 and [e is not None for e in haps].count(True) == 1
    x = [i for i, e in enumerate(haps) if e is not None][0]; e = haps[x]
    rc = pipeline.revcomp_str
    assert len(e["alleles"]) == 2 and e["alleles"].shape == (2, 3) and len(e["polished"]) == len(e["draft"]) == 2
    # the centre is in the orientation of the cluster that came first: the sites are 60, 200, 340 in that orientation
    fwd = res["centers"][x][3] in (T[0], T[1])
    assert e["sites"].tolist() == ([60, 200, 340] if fwd else [59, 199, 339])
    tmpl = [next((t for t in (0, 1) if p in (T[t], rc(T[t]))), None) for p in e["polished"]]
    assert sorted(tmpl) == [0, 1], "the polished haplotypes are not the two templates"
    # every placed read is in the haplotype it was generated from; the margin rule may leave out at most 10 % of the cluster's reads
    lists = [np.concatenate([np.nonzero(res["rep_of"] == r)[0] for r in c[4]]) for c in res["centers"]]
    org = origin[lists[x]]; asg = e["assign"]
    assert len(asg) == len(lists[x]) and set(org.tolist()) == {0, 1}
    for h in (0, 1):
        assert (org[asg == h] == tmpl[h]).all() and int((asg == h).sum()) == int(e["n_reads"][h])
    excluded = float((asg < 0).mean())
    print("excluded by the margin rule: %.4f of %d reads" % (excluded, len(asg)))
    assert excluded <= 0.10


def test_option_off_is_todays_result(oracle, three):
    T, sub, score, origin, kw = three
    plain = pipeline.run_hot_path(oracle, sub, score, **kw)
    off = pipeline.run_hot_path(oracle, sub, score, split_haplotypes=False, **kw)
    on = pipeline.run_hot_path(PhaseAdapter(oracle), sub, score, split_haplotypes=True, **kw)
    assert sorted(plain) == sorted(off) == ["centers", "counters", "hpc_err", "rep_of", "status"] and sorted(on) == sorted(list(plain) + ["haplotypes"])
    for r in (off, on):
        assert r["centers"] == plain["centers"]
        for key in ("rep_of", "status", "counters", "hpc_err"): assert np.array_equal(r[key], plain[key]), key


# the seeds of the false-split part of the sweep (tools/phase_sweep.py, profiles/phase.txt): the first three of its twenty
@pytest.mark.parametrize("seed", [5000, 5001, 5002])
def test_no_false_split_on_homopolymers(oracle, seed):
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("phase_sweep", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "phase_sweep.py"))
    sweep = importlib.util.module_from_spec(spec); spec.loader.exec_module(sweep)
    from ngspeciesid_amd import synth
    base = synth.make_species(1, sweep.L, 0.0, indel=0.0, seed=11)[0].tobytes().decode()
    hp = pc.with_homopolymers(base, sweep.RUNS)
    rs, _ = pc.pooled([hp], 300, 14.0, seed)
    api = PhaseAdapter(oracle)
    counts = api.consensus_support(ReadSet.from_strings([hp]), rs, [0, rs.n])[0]
    assert (np.sort(phase.allele_counts(counts, hp), axis=1)[:, -2] / np.maximum(counts[:, 0], 1)).max() > 0.08      # the runs do pile errors up at single columns
    assert phase.split(api, rs, hp, np.arange(rs.n, dtype=np.uint32), support=counts) is None


def test_flags(caplog):
    base = ["--ont", "--fastq", "x.fastq", "--outfolder", "o"]
    a = cli.build_parser().parse_args(base)
    assert a.split_haplotypes is False and (a.hap_min_alt_frac, a.hap_min_reads, a.hap_min_phi, a.hap_max) == tuple(phase.DEFAULTS[k] for k in ("min_alt_frac", "min_hap_reads", "min_phi", "max_haps"))
    b = cli.build_parser().parse_args(base + ["--split_haplotypes", "--hap_max", "4"])
    assert b.split_haplotypes is True and phase.policy_from_args(b)["max_haps"] == 4 and phase.check_args(b) is None
    b.hap_max = 17
    assert "hap_max" in phase.check_args(b)
    for argv in (["--ont", "--fastq_dir", ".", "--outfolder", "o"], base + ["--demux_sheet", "s.tsv"]):
        caplog.clear()
        with pytest.raises(SystemExit) as ex:
            cli.cli(argv + ["--consensus", "--split_haplotypes"])
        assert ex.value.code == 1 and "--split_haplotypes works on one sample" in caplog.text


def test_binding_without_the_symbols_is_an_error(oracle):
    from ngspeciesid_amd._capi import NgsidError
    with pytest.raises(NgsidError, match="phase_genotypes"):
        oracle.phase_pair_tables(np.zeros(0, np.uint8), [0, 0], [0, 0])


def test_table_rows():
    e = dict(sites=np.array([59, 199], dtype=np.uint32), alleles=np.array([[0, 4], [2, 3]], dtype=np.uint8), n_reads=np.array([150, 148]))
    assert phase.table_rows([17, 3], [None, e]) == [("3", "0", "150", "60,200", "A-"), ("3", "1", "148", "60,200", "GT")]


def test_cli_flag_adds_files_and_changes_no_other(oracle, tmp_path):
    """--split_haplotypes through the adapter: every file of the run without the flag, byte for byte, plus haplotypes.tsv and one FASTA per haplotype"""
    import os
    from ngspeciesid_amd import fastpath
    T = pc.three_templates()
    rs, _ = pc.pooled(T, 150, 17.0, pc.SPLIT_SEED)
    fq = str(tmp_path / "in.fastq")
    with open(fq, "w") as f:
        for i in range(rs.n):
            s, q = rs.get(i); f.write("@r%d\n%s\n+\n%s\n" % (i, s, q))
    runs = []
    for flag in ([], ["--split_haplotypes"]):
        out = str(tmp_path / ("o%d" % len(flag))); os.makedirs(out)
        args = cli.build_parser().parse_args(["--ont", "--fastq", fq, "--outfolder", out, "--t", "1", "--consensus", "--racon", "--racon_iter", "1", "--abundance_ratio", "0.05"] + flag); args.k, args.w = 13, 20
        fastpath.main(args, api=PhaseAdapter(oracle))
        runs.append({os.path.relpath(os.path.join(r, f), out): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(out) for f in fs})
    a, b = runs
    assert set(a) <= set(b) and all(a[f] == b[f] for f in a)
    rows = [r.split("\t") for r in b["haplotypes.tsv"].decode().splitlines()]
    assert rows[0] == ["cluster_id", "haplotype", "reads", "sites", "alleles"] and len(rows) == 3 and rows[1][0] == rows[2][0] and [r[1] for r in rows[1:]] == ["0", "1"]
    fas = [os.path.join("racon_cl_id_" + rows[1][0], "consensus_h%d.fasta" % j) for j in (0, 1)]
    assert sorted(set(b) - set(a)) == sorted(["haplotypes.tsv"] + fas)
    rc = pipeline.revcomp_str
    seqs = [b[fa].decode().split("\n")[1] for fa in fas]
    assert {next((t for t in (0, 1) if s in (T[t], rc(T[t]))), None) for s in seqs} == {0, 1}
    assert b[fas[0]].decode().startswith(">consensus_cl_id_%s_h0_total_supporting_reads_%s LN:i:400 RC:i:" % (rows[1][0], rows[1][2]))
