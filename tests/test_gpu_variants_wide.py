"""GPU: ngsid_ed_within_wide_batch and ngsid_near_pairs_wide (include/ngsid_near.h, csrc/k_near.hip: a band of 2, 4 or 8 words per lane) through Api.ed_within_wide /
Api.near_pairs_wide against tests/variants_reference.py.  Every comparison is exact equality.  K runs over the smallest and the largest bound of every band width.
The last tests run the policy layer (variants.py) with the wide bound on three samples of two 700-base templates 8 % apart, through variants.build and through the
command line."""
import os
import functools
import numpy as np
import pytest
import variants_reference as ref
import variants_cases as vc
from ngspeciesid_amd import runtime, variants
from ngspeciesid_amd._capi import ReadSet, NgsidError, NEAR_MAX_DIST, NEAR_WIDE_MAX_DIST, MAX_CONSENSUS_LEN

pytestmark = pytest.mark.gpu
KS = (32, 63, 64, 127, 128, 255)               # each band width (2, 4, 8 words) at its smallest and its largest bound


def _check_within(api, queries, targets, q_idx, t_idx, K, what, both=True):
    want = ref.ed_within(queries, targets, q_idx, t_idx, K, both)
    got = api.ed_within_wide(queries, targets, q_idx, t_idx, K, both_strands=both)
    for g, w, name in zip(got, want, ("dist", "strand")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: %s of pair %d (lengths %d, %d): got %d, want %d (%d places)" % (
            what, name, bad[0], len(queries[int(q_idx[bad[0]])]), len(targets[int(t_idx[bad[0]])]), g[bad[0]], w[bad[0]], len(bad))
    return got


def test_constants_are_the_headers():
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "ngsid_near.h")).read()
    assert "#define NGSID_NEAR_WIDE_MAX_DIST %d " % NEAR_WIDE_MAX_DIST in text and "#define NGSID_NEAR_MAX_DIST %d " % NEAR_MAX_DIST in text
    assert NEAR_MAX_DIST < NEAR_WIDE_MAX_DIST <= 255 and (NEAR_WIDE_MAX_DIST + 1) % 64 == 0          # 32 W - 1 edits of an even W; a distance fits the uint8 result
    assert all(K <= NEAR_WIDE_MAX_DIST for K in KS)


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
        for n in (K + 2, 650):
            a, b = vc.at_distance(rng, n, k); qs.append(a); ts.append(b)                 # distance exactly K and exactly K + 1
            for where in ("lead", "trail", "mid"):                                       # length difference exactly K / K + 1: k leading deletions, k trailing insertions
                a, b = vc.indel_only(rng, n, k, where)
                qs += [a, b]; ts += [b, a]
    idx = np.arange(len(qs))
    got = _check_within(gpu_api, qs, ts, idx, idx, K, "K=%d" % K, both=False)
    assert sorted(set(got[0].tolist())) == [-1, K]
    _check_within(gpu_api, qs, ts, idx, idx, K, "K=%d both strands" % K)


@pytest.mark.parametrize("K", KS)
def test_carry_chain_of_poly_a(gpu_api, K):
    """poly-A against poly-A: Eq and VP are all ones inside the sequences, so the sum carries through every word of the band in every column"""
    n = 600
    qs = ["A" * n] * 4 + ["A" * (n + d) for d in (1, K, K + 1)] + ["A" * n, "A" * 300 + "G" + "A" * 299]
    ts = ["A" * (n + d) for d in (0, 1, K, K + 1)] + ["A" * n] * 3 + ["A" * 300 + "G" + "A" * 299, "A" * n]
    idx = np.arange(len(qs))
    got = _check_within(gpu_api, qs, ts, idx, idx, K, "K=%d poly-A" % K, both=False)
    assert got[0].tolist() == [0, 1, K, -1, 1, K, -1, 1, 1]
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
    for K in (32, NEAR_WIDE_MAX_DIST):
        got = _check_within(gpu_api, qs, ts, idx, idx, K, "K=%d" % K)
        _check_within(gpu_api, qs, ts, idx, idx, K, "K=%d forward only" % K, both=False)
        assert got[0][:5].tolist() == [0, 1, 0, 2, 0] and got[1][:5].tolist() == [0, 0, 0, 0, 0]      # N equals N only; the palindrome is on strand 0
        assert got[1][5:9].tolist() == [1, 1, 0, 1] and (got[0][5:9] >= 0).all()                      # near on the reverse strand only
        assert got[0][10:13].tolist() == [0, 3, 3]                                                    # empty sequences
    one = gpu_api.ed_within_wide(qs, ts, idx, idx, 32, both_strands=False)
    assert one[0][5] == -1 and one[0][6] == -1 and (one[1] == 0).all()


@pytest.mark.parametrize("n_pairs", [0, 1, 63, 64, 65, 300])
def test_pair_counts_with_mixed_lengths(gpu_api, n_pairs):
    """lanes of one wave finish at different columns: lengths 0 .. 400, related and unrelated pairs, indices into two different sets in random order"""
    rng = np.random.default_rng(200 + n_pairs)
    qs, ts = [], []
    for p in range(max(n_pairs // 2, 1)):
        la = int(rng.choice([0, 1, 5, 40, 64, 100, 257, 400])); lb = max(la + int(rng.integers(-9, 10)), 0)
        a, b = vc.related_pair(rng, la, lb, int(rng.integers(0, 45)))
        qs.append(a); ts.append(b if p % 3 else ref.rc(b))
    qi = rng.integers(0, len(qs), n_pairs); ti = np.where(rng.random(n_pairs) < 0.7, qi, rng.integers(0, len(ts), n_pairs))
    got = _check_within(gpu_api, qs, ts, qi, ti, 40, "%d pairs" % n_pairs)
    assert got[0].shape == (n_pairs,)
    if n_pairs >= 63: assert (got[0] > NEAR_MAX_DIST).any() and (got[0] < 0).any()


@pytest.mark.parametrize("K", (0, NEAR_MAX_DIST))
def test_below_32_the_wide_calls_are_the_one_word_calls(gpu_api, K):
    """byte for byte what ed_within and near_pairs return on the same input"""
    qs, ts = _grid(32)
    idx = np.arange(len(qs))
    for both in (True, False):
        a, b = gpu_api.ed_within(qs, ts, idx, idx, K, both_strands=both), gpu_api.ed_within_wide(qs, ts, idx, idx, K, both_strands=both)
        assert all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))
        seqs = list(_family_set()[0])
        a, b = gpu_api.near_pairs(seqs, K, both_strands=both), gpu_api.near_pairs_wide(seqs, K, both_strands=both)
        assert all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert len(a[0]) > 0


def test_one_pair_of_the_largest_size(gpu_api):
    """the expected values are known by construction (vc.at_distance): no reference DP of 16384 x 16384"""
    rng = np.random.default_rng(7)
    K = NEAR_WIDE_MAX_DIST
    a, b = vc.at_distance(rng, MAX_CONSENSUS_LEN, K)
    c, d = vc.at_distance(rng, MAX_CONSENSUS_LEN, K + 1)
    dist, strand = gpu_api.ed_within_wide([a, c], [b, d], [0, 1], [0, 1], K, both_strands=False)
    assert dist.tolist() == [K, -1] and strand.tolist() == [0, 0]
    assert [tuple(int(v[0]) for v in gpu_api.near_pairs_wide([x, y], K, both_strands=False)) if k == K else len(gpu_api.near_pairs_wide([x, y], K, both_strands=False)[0])
            for x, y, k in ((a, b, K), (c, d, K + 1))] == [(0, 1, K, 0), 0]


# ---- all pairs
FAMILY_KS = (40, 100)


@functools.lru_cache(maxsize=None)
def _family_set():
    """129 sequences of about 200 bases: six families whose roots are 15 - 30 % off the first, members 4 % off their root and cut or grown at the end so that the
    lengths spread by more than either K; three exact duplicates, a reverse-complemented member and an empty sequence
    -> (sequences, {K: the brute-force pairs at max_dist K}, every pair the reference puts within 2 K_max, the forward-only pairs at K_max)"""
    rng = np.random.default_rng(131)
    roots = [vc.rand_seq(rng, 200)]
    for f in range(1, 6): roots.append(vc.mutate(rng, roots[0], 0.15 + 0.03 * f))
    seqs = []
    for m in range(22):
        for f, r in enumerate(roots):
            q = r if m == 0 else vc.mutate(rng, r, 0.04)
            if m % 5 == 3: q = q[:len(q) - int(rng.integers(20, 130))]
            if m % 7 == 4: q = q + vc.rand_seq(rng, int(rng.integers(10, 60)))
            seqs.append(q)
    seqs = seqs[:129]
    seqs[7] = seqs[2]; seqs[64] = seqs[2]; seqs[128] = seqs[63]
    seqs[11] = ref.rc(seqs[11]); seqs[70] = ref.rc(seqs[70]); seqs[40] = ""
    far = ref.near_pairs(seqs, 2 * max(FAMILY_KS))
    return tuple(seqs), {K: tuple(p for p in far if p[2] <= K) for K in FAMILY_KS}, tuple(far), tuple(ref.near_pairs(seqs, max(FAMILY_KS), False))


def _pairs(res):
    return [tuple(int(v) for v in row) for row in zip(*res)]


def test_the_family_set_straddles_the_bounds():
    """on the reference's own result: pairs between 32 and K, pairs beyond K, both strands, duplicates, lengths spread by more than K"""
    seqs, full, far, _ = _family_set()
    lens = [len(s) for s in seqs]
    assert len(seqs) == 129 and max(lens) - min(l for l in lens if l) > max(FAMILY_KS) and min(lens) == 0
    for K in FAMILY_KS:
        assert sum(1 for p in full[K] if NEAR_MAX_DIST < p[2] <= K) >= 20, K
        assert sum(1 for p in far if p[2] > K) >= 20, K
        assert any(p[3] for p in full[K]) and any(p[2] == 0 for p in full[K])


@pytest.mark.parametrize("K", FAMILY_KS)
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_near_pairs_against_brute_force(gpu_api, n, K):
    seqs, full, _, forward = _family_set()
    want = [p for p in full[K] if p[1] < n]
    res = gpu_api.near_pairs_wide(list(seqs[:n]), K)
    assert [a.dtype for a in res] == [np.uint32, np.uint32, np.uint8, np.uint8]
    assert _pairs(res) == want
    if n == 129:
        fwd = gpu_api.near_pairs_wide(list(seqs), K, both_strands=False)
        assert _pairs(fwd) == [p for p in forward if p[2] <= K]


def test_cap_and_needed(gpu_api):
    seqs, full = _family_set()[:2]
    for K in FAMILY_KS:
        n = len(full[K])
        assert _pairs(gpu_api.near_pairs_wide(list(seqs), K)) == list(full[K])                       # cap=None: the count call, then the fill call
        assert _pairs(gpu_api.near_pairs_wide(list(seqs), K, cap=n)) == list(full[K]) and _pairs(gpu_api.near_pairs_wide(list(seqs), K, cap=n + 100)) == list(full[K])
        for cap in (0, 1, n - 1):
            with pytest.raises(NgsidError) as e:
                gpu_api.near_pairs_wide(list(seqs), K, cap=cap)
            assert e.value.code == -4 and e.value.needed == n
    far = [vc.rand_seq(np.random.default_rng(s), 120) for s in range(4)]
    assert _pairs(gpu_api.near_pairs_wide(far, 40, cap=0)) == [] and _pairs(gpu_api.near_pairs_wide(far, 40)) == []
    assert _pairs(gpu_api.near_pairs_wide(list(seqs), 40)) == list(full[40])                         # the context is usable after every refusal


def test_chunking_and_residence():
    seqs, full = _family_set()[:2]
    qs, ts = _grid(64)
    idx = np.arange(len(qs))
    want = ref.ed_within(qs, ts, idx, idx, 64)
    with runtime.new_api() as api:
        for val in (1, 7, 0):
            api.set_option("near_chunk_seqs", val)
            for K in FAMILY_KS:
                assert _pairs(api.near_pairs_wide(list(seqs), K)) == list(full[K]), "near_chunk_seqs=%d K=%d" % (val, K)
        for val in (1, 100, 0):
            api.set_option("near_chunk_pairs", val)
            got = api.ed_within_wide(qs, ts, idx, idx, 64)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "near_chunk_pairs=%d" % val
        dev = api.upload_reads(ReadSet.from_strings(list(seqs)))
        try:
            assert _pairs(api.near_pairs_wide(dev, 100)) == list(full[100]), "device-resident read set"
        finally:
            dev.release()
        api.set_option("release_scratch", 1)
        assert _pairs(api.near_pairs_wide(list(seqs), 100)) == list(full[100]), "after release_scratch"
        api.profile_enable(True); api.profile_read()
        api.near_pairs_wide(list(seqs), 100, cap=len(full[100])); api.ed_within_wide(qs[:4], ts[:4], idx[:4], idx[:4], 64)
        prof = api.profile_read()[0]
        api.profile_enable(False)
        assert "k_near_tiles_wide" in prof and "k_near_within_wide" in prof and "k_near_tiles" not in prof and "k_near_within" not in prof


def test_errors_come_back_as_return_codes(gpu_api):
    a, b = "ACGTTGCATGCCGATAGGCTTAACGG", "TTGACCGGTAACGTTAGCATCGGCTA"
    long_ = "ACGT" * (MAX_CONSENSUS_LEN // 4) + "A"
    for fn, code in ((lambda: gpu_api.near_pairs_wide([a, b], NEAR_WIDE_MAX_DIST + 1), -2), (lambda: gpu_api.near_pairs_wide([a, b], -1), -2),
                     (lambda: gpu_api.near_pairs_wide([a, b[:5] + "c" + b[6:]], 40), -3), (lambda: gpu_api.near_pairs_wide([a, long_], 40), -6),
                     (lambda: gpu_api.ed_within_wide([a], [b], [0], [0], NEAR_WIDE_MAX_DIST + 1), -2), (lambda: gpu_api.ed_within_wide([a], [b], [0], [0], -1), -2),
                     (lambda: gpu_api.ed_within_wide([a], [b], [0], [1], 40), -2), (lambda: gpu_api.ed_within_wide([a], [b], [1], [0], 40), -2),
                     (lambda: gpu_api.ed_within_wide([a[:3] + "t" + a[4:]], [b], [0], [0], 40), -3), (lambda: gpu_api.ed_within_wide([a], [long_], [0], [0], 40), -6)):
        with pytest.raises(NgsidError) as e:
            fn()
        assert e.value.code == code
    # the one-word calls keep their range
    with pytest.raises(NgsidError) as e:
        gpu_api.near_pairs([a, b], NEAR_MAX_DIST + 1)
    assert e.value.code == -2
    assert _pairs(gpu_api.near_pairs_wide([a, a], 40)) == [(0, 1, 0, 0)] and gpu_api.ed_within_wide([a], [b], [0], [0], 40)[0].tolist() == [ref.D(a, b)[0]]


# ---- end to end: two 700-base templates 8 % apart in three samples, one sample reverse-complemented
def _two_template_groups():
    rng = np.random.default_rng(17)
    a = vc.rand_seq(rng, 700)
    b = list(a)
    for p in rng.choice(700, size=56, replace=False): b[int(p)] = "ACGT"[("ACGT".index(b[int(p)]) + 1 + int(rng.integers(0, 3))) % 4]
    b = "".join(b)
    groups = []
    for s in range(3):
        cons = []
        for f, root in enumerate((a, b)):
            q = root if s == 0 else vc.mutate(rng, root, 0.004)
            if s == 1: q = ref.rc(q)
            cons.append(("consensus_cl_id_%d_total_supporting_reads_%d" % (f, 40 - 10 * s - 3 * f), 40 - 10 * s - 3 * f, q))
        groups.append(("sample_%d" % s, None, cons))
    return groups


def _reference_table(col, identity, K):
    lengths = [len(s) for s in col["seqs"]]
    return ref.cluster(col["sizes"], lengths, col["seqs"], ref.near_pairs(col["seqs"], K), ref.thresholds(lengths, identity, K))


def test_build_and_the_command_line_with_the_wide_bound(gpu_api, tmp_path):
    from ngspeciesid_amd.cli import cli
    groups = _two_template_groups()
    col = variants.collect(groups)
    want = _reference_table(col, "0.9", 80)
    assert len(want[1]) == 1 and max(want[2]) > NEAR_MAX_DIST and 1 in want[3]
    tab = variants.build(gpu_api, col, identity="0.9", wide_max_dist=80)
    assert tab["variant_of"].tolist() == want[0] and tab["dist"].tolist() == want[2] and tab["strand"].tolist() == want[3]
    assert len(tab["variants"]) == 1 and tab["counts"].tolist() == [[sum(nr for _, nr, _ in g[2]) for g in groups]]
    narrow = variants.build(gpu_api, col, identity="0.9")
    assert narrow["variant_of"].tolist() == _reference_table(col, "0.9", NEAR_MAX_DIST)[0] and len(narrow["variants"]) == 2
    paths = []
    for name, _, cons in groups:
        paths.append(str(tmp_path / (name + ".fasta")))
        with open(paths[-1], "w") as fh:
            for cid, _, q in cons: fh.write(">%s\n%s\n" % (cid, q))
    with pytest.raises(SystemExit) as e:
        cli(["variants", "--fasta"] + paths + ["--outfolder", str(tmp_path / "out"), "--variant_identity", "0.9", "--variant_wide_max_dist", "80"])
    assert e.value.code == 0
    assert sorted(os.listdir(tmp_path / "out")) == ["variant_members.tsv", "variant_table.tsv", "variants.fasta"]
    assert variants.read_table(str(tmp_path / "out" / "variant_members.tsv")) == tab["members"]
    rows = variants.read_table(str(tmp_path / "out" / "variant_table.tsv"))
    assert [[r[s] for s in tab["samples"]] for r in rows] == tab["counts"].tolist()
    assert open(tmp_path / "out" / "variants.fasta").read() == ">variant_0;size=%d;samples=3\n%s\n" % (int(col["sizes"].sum()), col["seqs"][want[1][0]])
