"""GPU: ngsid_ed_within_batch and ngsid_near_pairs (include/ngsid_near.h, csrc/k_near.hip) through Api.ed_within / Api.near_pairs against tests/variants_reference.py.
Every comparison is exact equality.  The last tests run the policy layer (variants.py) on reads of three amplicons in three samples, one of them reverse-complemented,
through pipeline.run_hot_path_samples and through the command line."""
import os
import functools
import numpy as np
import pytest
import variants_reference as ref
import variants_cases as vc
from ngspeciesid_amd import runtime, variants
from ngspeciesid_amd._capi import ReadSet, NgsidError, NEAR_MAX_DIST, MAX_CONSENSUS_LEN

pytestmark = pytest.mark.gpu
KS = (0, 1, 15, 31)


def _check_within(api, queries, targets, q_idx, t_idx, K, what, both=True):
    want = ref.ed_within(queries, targets, q_idx, t_idx, K, both)
    got = api.ed_within(queries, targets, q_idx, t_idx, K, both_strands=both)
    for g, w, name in zip(got, want, ("dist", "strand")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: %s of pair %d (lengths %d, %d): got %d, want %d (%d places)" % (
            what, name, bad[0], len(queries[int(q_idx[bad[0]])]), len(targets[int(t_idx[bad[0]])]), g[bad[0]], w[bad[0]], len(bad))
    return got


def test_constants_are_the_headers():
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "ngsid_near.h")).read()
    assert "#define NGSID_NEAR_MAX_DIST %d " % NEAR_MAX_DIST in text and NEAR_MAX_DIST == 31 and "#define NGSID_NEAR_BOTH_STRANDS 1u" in text


@functools.lru_cache(maxsize=None)
def _grid(K):
    """related pairs at every length pair of the border set (and 650) whose distance the reference puts at K + 2 at the most: both sides of the bound"""
    rng = np.random.default_rng(40 + K)
    L = vc.LENGTHS(K) + [650]
    qs, ts = [], []
    for la in L:
        for lb in L:
            if abs(la - lb) > K + 2: continue
            room = K - abs(la - lb)
            for e in sorted({0, max(room // 2, 0), max(room, 0), room + 2}):
                if e < 0: continue
                a, b = vc.related_pair(rng, la, lb, e)
                if ref.D(a, b)[0] <= K + 2: qs.append(a); ts.append(b)
    return qs, ts


@pytest.mark.parametrize("K", KS)
def test_lengths_at_the_kernels_borders(gpu_api, K):
    qs, ts = _grid(K)
    idx = np.arange(len(qs))
    got = _check_within(gpu_api, qs, ts, idx, idx, K, "K=%d" % K)
    assert (got[0] >= 0).sum() >= 8 and (got[0] < 0).any()
    _check_within(gpu_api, qs, ts, idx, idx, K, "K=%d forward only" % K, both=False)
    _check_within(gpu_api, ts, qs, idx, idx, K, "K=%d the other way round" % K)


@pytest.mark.parametrize("K", KS)
def test_exact_distance_length_difference_and_outermost_diagonal(gpu_api, K):
    rng = np.random.default_rng(60 + K)
    qs, ts = [], []
    for k in (K, K + 1):
        for n in (64, 300, 650):
            a, b = vc.at_distance(rng, n, k); qs.append(a); ts.append(b)                 # distance exactly K and exactly K + 1
            for where in ("lead", "trail", "mid"):                                       # length difference exactly K / K + 1: k leading deletions, k trailing insertions
                a, b = vc.indel_only(rng, n, k, where)
                qs += [a, b]; ts += [b, a]
    idx = np.arange(len(qs))
    got = _check_within(gpu_api, qs, ts, idx, idx, K, "K=%d" % K, both=False)
    assert sorted(set(got[0].tolist())) == [-1, K]
    _check_within(gpu_api, qs, ts, idx, idx, K, "K=%d both strands" % K)


@pytest.mark.parametrize("K", (0, 1, 31))
def test_carry_chain_of_poly_a(gpu_api, K):
    """poly-A against poly-A: Eq and VP are all ones inside the sequences, so the sum carries out of the band word in every column; 600 bases, so the words loaded
    one block ahead are used.  The true distances are 0, 1, K, K + 1, 1, K, K + 1, 1, 1: [0, 1, K, -1, 1, K, -1, 1, 1] for K >= 1, and at K = 0 the 1s are beyond
    the bound as well"""
    n = 600
    qs = ["A" * n] * 4 + ["A" * (n + d) for d in (1, K, K + 1)] + ["A" * n, "A" * 300 + "G" + "A" * 299]
    ts = ["A" * (n + d) for d in (0, 1, K, K + 1)] + ["A" * n] * 3 + ["A" * 300 + "G" + "A" * 299, "A" * n]
    idx = np.arange(len(qs))
    got = _check_within(gpu_api, qs, ts, idx, idx, K, "K=%d poly-A" % K, both=False)
    assert got[0].tolist() == ([0, 1, K, -1, 1, K, -1, 1, 1] if K >= 1 else [0, -1, 0, -1, -1, 0, -1, -1, -1])
    _check_within(gpu_api, qs, ts, idx, idx, K, "K=%d poly-A both strands" % K)


def test_letters_palindromes_and_the_reverse_strand(gpu_api):
    rng = np.random.default_rng(9)
    pal = "ACGTTAACGT"
    assert ref.rc(pal) == pal
    a = vc.rand_seq(rng, 200); b = vc.mutate(rng, a, 0.04)
    n5 = vc.rand_seq(rng, 90, "ACGTN")
    qs = ["N", "N", "ANNA", "ANNA", pal, a, ref.rc(a), a, n5, n5, "", "", "ACG", a + "T"]
    ts = ["N", "A", "ANNA", "AAAA", pal, ref.rc(b), b, b, ref.rc(n5), vc.mutate(rng, n5, 0.05), "", "ACG", "", ref.rc(a)]
    idx = np.arange(len(qs))
    for K in (0, 3, 31):
        got = _check_within(gpu_api, qs, ts, idx, idx, K, "K=%d" % K)
        _check_within(gpu_api, qs, ts, idx, idx, K, "K=%d forward only" % K, both=False)
    assert got[0][:5].tolist() == [0, 1, 0, 2, 0] and got[1][:5].tolist() == [0, 0, 0, 0, 0]      # N equals N only; the palindrome is on strand 0
    assert got[1][5:9].tolist() == [1, 1, 0, 1] and (got[0][5:9] >= 0).all()                      # near on the reverse strand only
    one = gpu_api.ed_within(qs, ts, idx, idx, 31, both_strands=False)
    assert one[0][5] == -1 and one[0][6] == -1 and (one[1] == 0).all()


@pytest.mark.parametrize("n_pairs", [0, 1, 63, 64, 65, 300])
def test_pair_counts_with_mixed_lengths(gpu_api, n_pairs):
    """lanes of one wave finish at different columns: lengths 0 .. 400, related and unrelated pairs, indices into two different sets in random order"""
    rng = np.random.default_rng(200 + n_pairs)
    qs, ts = [], []
    for p in range(max(n_pairs // 2, 1)):
        la = int(rng.choice([0, 1, 5, 40, 64, 100, 257, 400])); lb = max(la + int(rng.integers(-3, 4)), 0)
        a, b = vc.related_pair(rng, la, lb, int(rng.integers(0, 12)))
        qs.append(a); ts.append(b if p % 3 else ref.rc(b))
    qi = rng.integers(0, len(qs), n_pairs); ti = np.where(rng.random(n_pairs) < 0.7, qi, rng.integers(0, len(ts), n_pairs))
    got = _check_within(gpu_api, qs, ts, qi, ti, 12, "%d pairs" % n_pairs)
    assert got[0].shape == (n_pairs,)
    if n_pairs >= 63: assert (got[0] >= 0).any() and (got[0] < 0).any()


def test_one_pair_of_the_largest_size(gpu_api):
    rng = np.random.default_rng(7)
    L = MAX_CONSENSUS_LEN
    a = vc.rand_seq(rng, L)
    b = list(a)
    for p in rng.choice(L, size=31, replace=False): b[int(p)] = "ACGT"[("ACGT".index(b[int(p)]) + 1) % 4]
    b = "".join(b)
    c = b[:5000] + b[5001:] + "A"                                   # one deletion and one insertion 11 000 columns apart on top
    got = _check_within(gpu_api, [a], [b, c], [0, 0], [0, 1], 31, "16384 x 16384", both=False)
    assert 29 <= got[0][0] <= 31 and got[0][1] == -1


# ---- all pairs
@functools.lru_cache(maxsize=None)
def _family_set():
    """130 sequences of about 80 bases: five families whose roots are 10 % apart, members 3 % off their root, so that some pairs are near and some are not; three
    exact duplicates, a reverse-complemented member and an empty sequence -> (sequences, the brute-force pairs at max_dist 8)"""
    rng = np.random.default_rng(31)
    seqs, _ = vc.families(rng, 5, 26, 80, 0.03, between=0.10)
    seqs[7] = seqs[2]; seqs[64] = seqs[2]; seqs[129] = seqs[63]
    seqs[11] = ref.rc(seqs[11]); seqs[70] = ref.rc(seqs[70]); seqs[40] = ""
    return tuple(seqs), tuple(ref.near_pairs(seqs, 8))


def _pairs(res):
    return [tuple(int(v) for v in row) for row in zip(*res)]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 130])
def test_near_pairs_against_brute_force(gpu_api, n):
    seqs, full = _family_set()
    want = [p for p in full if p[1] < n]
    res = gpu_api.near_pairs(list(seqs[:n]), 8)
    assert [a.dtype for a in res] == [np.uint32, np.uint32, np.uint8, np.uint8]
    assert _pairs(res) == want
    if n == 130:
        assert 200 < len(want) < 130 * 129 // 4 and any(p[3] for p in want) and any(p[2] == 0 for p in want)
        fwd = gpu_api.near_pairs(list(seqs), 8, both_strands=False)
        assert _pairs(fwd) == ref.near_pairs(list(seqs), 8, False)
        for K in (0, 3):
            assert _pairs(gpu_api.near_pairs(list(seqs), K)) == [p for p in full if p[2] <= K]


def test_a_permuted_set_gives_the_same_pairs(gpu_api):
    seqs, full = _family_set()
    perm = np.random.default_rng(3).permutation(len(seqs))                        # position x of the permuted set holds sequence perm[x]
    got = _pairs(gpu_api.near_pairs([seqs[int(p)] for p in perm], 8))
    assert got == sorted(got) and len({g[:2] for g in got}) == len(got)
    back = sorted((min(int(perm[i]), int(perm[j])), max(int(perm[i]), int(perm[j])), d, s) for i, j, d, s in got)
    assert back == list(full)


def test_cap_and_needed(gpu_api):
    seqs, full = _family_set()
    n = len(full)
    assert _pairs(gpu_api.near_pairs(list(seqs), 8, cap=n)) == list(full) and _pairs(gpu_api.near_pairs(list(seqs), 8, cap=n + 100)) == list(full)
    for cap in (0, 1, n - 1):
        with pytest.raises(NgsidError) as e:
            gpu_api.near_pairs(list(seqs), 8, cap=cap)
        assert e.value.code == -4 and e.value.needed == n
    far = [vc.rand_seq(np.random.default_rng(s), 60) for s in range(4)]
    assert _pairs(gpu_api.near_pairs(far, 8, cap=0)) == [] and _pairs(gpu_api.near_pairs(far, 8)) == []
    assert _pairs(gpu_api.near_pairs(list(seqs), 8)) == list(full)                # the context is usable after every refusal


def test_chunking_and_residence():
    seqs, full = _family_set()
    qs, ts = _grid(15)
    idx = np.arange(len(qs))
    want = ref.ed_within(qs, ts, idx, idx, 15)
    with runtime.new_api() as api:
        for val in (1, 7, 0):
            api.set_option("near_chunk_seqs", val)
            assert _pairs(api.near_pairs(list(seqs), 8)) == list(full), "near_chunk_seqs=%d" % val
        for val in (1, 100, 0):
            api.set_option("near_chunk_pairs", val)
            got = api.ed_within(qs, ts, idx, idx, 15)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "near_chunk_pairs=%d" % val
        dev = api.upload_reads(ReadSet.from_strings(list(seqs)))
        try:
            assert _pairs(api.near_pairs(dev, 8)) == list(full), "device-resident read set"
        finally:
            dev.release()
        api.set_option("release_scratch", 1)
        assert _pairs(api.near_pairs(list(seqs), 8)) == list(full), "after release_scratch"


@pytest.mark.parametrize("max_tiles", [1, 7, 64])
def test_the_tile_cap_of_a_launch_does_not_change_the_result(gpu_api, max_tiles):
    """near_max_tiles lowers the tiles one launch takes: the rows are split as they are beyond the real bound of a launch (tests/test_gpu_launch_bound.py), a row of
    more tiles than the cap still goes in one launch.  The 130 sequences have up to three tiles a row."""
    seqs, full = _family_set()
    try:
        gpu_api.set_option("near_max_tiles", max_tiles)
        assert _pairs(gpu_api.near_pairs(list(seqs), 8)) == list(full)
    finally:
        gpu_api.set_option("near_max_tiles", 0)
        gpu_api.set_option("release_scratch", 1)


def test_errors_come_back_as_return_codes(gpu_api):
    a, b = "ACGTTGCATGCCGATAGGCTTAACGG", "TTGACCGGTAACGTTAGCATCGGCTA"
    long_ = "ACGT" * (MAX_CONSENSUS_LEN // 4) + "A"
    for fn, code in ((lambda: gpu_api.near_pairs([a, b], NEAR_MAX_DIST + 1), -2), (lambda: gpu_api.near_pairs([a, b], -1), -2),
                     (lambda: gpu_api.near_pairs([a, b[:5] + "c" + b[6:]], 3), -3), (lambda: gpu_api.near_pairs([a, long_], 3), -6),
                     (lambda: gpu_api.ed_within([a], [b], [0], [0], NEAR_MAX_DIST + 1), -2), (lambda: gpu_api.ed_within([a], [b], [0], [1], 3), -2),
                     (lambda: gpu_api.ed_within([a], [b], [1], [0], 3), -2), (lambda: gpu_api.ed_within([a[:3] + "t" + a[4:]], [b], [0], [0], 3), -3),
                     (lambda: gpu_api.ed_within([a], [long_], [0], [0], 3), -6)):
        with pytest.raises(NgsidError) as e:
            fn()
        assert e.value.code == code
    assert _pairs(gpu_api.near_pairs([a, a], 0)) == [(0, 1, 0, 0)] and gpu_api.ed_within([a], [a], [0], [0], 0)[0].tolist() == [0]


# ---- end to end: three amplicons in three samples, one sample reverse-complemented
def _sample_reads():
    """amplicon 0 in all three samples, amplicon 1 in two, amplicon 2 in one; every read of sample 1 is reverse-complemented.  The read counts are uneven so that
    no consensus of the flipped sample is the most abundant of its variant: its members are then on strand 1.  -> [reads dict per sample], the amplicons"""
    from ngspeciesid_amd import synth
    sp = synth.make_species(3, 400, 0.15, seed=2)
    plan = (([0, 1, 2], [0.3, 0.4, 0.3], 200, 0.0), ([0, 1], [0.5, 0.5], 100, 1.0), ([0], [1.0], 150, 0.0))
    return [synth.make_reads([sp[x] for x in which], n, mu=17.0, seed=20 + s, abundance=ab, rc_fraction=rcf) for s, (which, ab, n, rcf) in enumerate(plan)], sp


def _assert_the_three_variants(tab, centers_per_sample):
    """exactly three variants (3, 2 and 1 samples); every cell is the supporting-read count of the consensus it came from; the flipped sample's members are on strand 1"""
    assert len(tab["variants"]) == 3 and sorted(v["n_samples"] for v in tab["variants"]) == [1, 2, 3]
    assert [len(c) for c in centers_per_sample] == [3, 2, 1]
    at = 0
    for s, cen in enumerate(centers_per_sample):
        for nr in cen:
            m = tab["members"][at]; v = int(m["variant"].split("_")[1])
            assert m["reads"] == nr and tab["counts"][v, s] == nr and m["strand"] == ("-" if s == 1 else "+") and m["dist"] <= 12
            at += 1
    assert int(tab["counts"].sum()) == sum(nr for cen in centers_per_sample for nr in cen) and int((tab["counts"] > 0).sum()) == 6


def test_run_hot_path_samples_builds_the_table(gpu_api):
    from ngspeciesid_amd import pipeline
    from ngspeciesid_amd.ptable import select_p_table
    from ngspeciesid_amd.hostutil import subset_reads
    rds, _ = _sample_reads()
    parts, scores = [], []
    for rd in rds:
        rs = ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64))
        score, _, keep = gpu_api.score_reads(rs, 13, 7.0)
        idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
        parts.append(subset_reads(rs, idx)); scores.append(score[idx])
    lens = np.concatenate([np.diff(p.off.astype(np.int64)) for p in parts])
    allr = ReadSet(np.concatenate([p.seq for p in parts]), np.concatenate([p.qual for p in parts]), np.concatenate(([0], np.cumsum(lens))).astype(np.uint64))
    seg = np.concatenate(([0], np.cumsum([p.n for p in parts])))
    kw = dict(acc_rank=np.concatenate([np.arange(p.n) for p in parts]).astype(np.uint32), k=13, w=20, abundance_ratio=0.1, racon_iter=2, p_shared=select_p_table(13, 20))
    res = pipeline.run_hot_path_samples(gpu_api, allr, np.concatenate(scores), seg, variants=True, **kw)
    plain = pipeline.run_hot_path_samples(gpu_api, allr, np.concatenate(scores), seg, **kw)
    assert all("variants" not in o for o in plain) and [[c[:4] for c in o["centers"]] for o in plain] == [[c[:4] for c in o["centers"]] for o in res]
    tab = res[0]["variants"]["table"]
    assert all(o["variants"]["table"] is tab for o in res)
    _assert_the_three_variants(tab, [[c[0] for c in o["centers"]] for o in res])
    for s, o in enumerate(res):
        assert [m["strand"] for m in o["variants"]["members"]] == [1 if s == 1 else 0] * len(o["centers"])
    # the table is what the policy layer makes of the final sequences through one near-pairs call
    groups = [(s, None, [(c[1], c[0], c[3]) for c in o["centers"]]) for s, o in enumerate(res)]
    again = variants.build(gpu_api, variants.collect(groups))
    assert again["members"] == tab["members"] and np.array_equal(again["counts"], tab["counts"])
    assert all(o["variants"] is None for o in pipeline.run_hot_path_samples(gpu_api, allr, np.concatenate(scores), seg, do_consensus=False, variants=True, **kw))


def _files(folder):
    out = {}
    for root, _, fs in os.walk(folder):
        for f in fs:
            out[os.path.relpath(os.path.join(root, f), folder)] = open(os.path.join(root, f), "rb").read()
    return out


def test_cli_fastq_dir_writes_the_three_files(gpu_api, tmp_path):
    from ngspeciesid_amd.cli import cli
    from ngspeciesid_amd import synth
    d = tmp_path / "in"; d.mkdir()
    rds, _ = _sample_reads()
    for name, rd in zip(("s_a", "s_b", "s_c"), rds):
        synth.reads_to_fastq(rd, str(d / (name + ".fastq")), prefix=name)
    flags = ["--ont", "--fastq_dir", str(d), "--t", "1", "--consensus", "--racon", "--racon_iter", "2", "--abundance_ratio", "0.1"]
    cli(flags + ["--outfolder", str(tmp_path / "A"), "--variants"])
    cli(flags + ["--outfolder", str(tmp_path / "B")])
    got, plain = _files(str(tmp_path / "A")), _files(str(tmp_path / "B"))
    assert sorted(k for k in got if k not in plain) == ["variant_members.tsv", "variant_table.tsv", "variants.fasta"]
    assert all(got[k] == plain[k] for k in plain if not k.endswith("logfile.txt"))
    members = variants.read_table(str(tmp_path / "A" / "variant_members.tsv"))
    rows = variants.read_table(str(tmp_path / "A" / "variant_table.tsv"))
    names = ["s_a", "s_b", "s_c"]
    tab = dict(variants=[dict(n_samples=sum(r[s] > 0 for s in names)) for r in rows], members=members, counts=np.array([[r[s] for s in names] for r in rows]))
    _assert_the_three_variants(tab, [[m["reads"] for m in members if m["sample"] == s] for s in names])
    assert [l[1:].split(";")[0] for l in got["variants.fasta"].decode().splitlines()[0::2]] == [r["variant"] for r in rows]
    # the sub-command over the run's own consensus files, one FASTA per sample, writes the same three files
    for s in names:
        with open(tmp_path / (s + ".fasta"), "w") as fh:
            for m in members:
                if m["sample"] == s: fh.write(got["%s/racon_cl_id_%s/consensus.fasta" % (s, m["consensus id"].split("_")[3])].decode())
    with pytest.raises(SystemExit) as e:
        cli(["variants", "--fasta"] + [str(tmp_path / (s + ".fasta")) for s in names] + ["--outfolder", str(tmp_path / "C")])
    assert e.value.code == 0
    sub = _files(str(tmp_path / "C"))
    assert sorted(sub) == ["variant_members.tsv", "variant_table.tsv", "variants.fasta"] and all(sub[k] == got[k] for k in sub)
