"""GPU: ngsid_hp_runs (include/ngsid_hp.h) through the C-ABI == its definition restated from the oracle's parts (tests/hp_reference.py), histogram for histogram and
strand for strand, and the pipeline / CLI layers on top of it.  The shapes are small on purpose: every case is an edge of the path matrix, the position matrix or the kernel."""
import os
import numpy as np
import pytest
from ngspeciesid_amd import synth, pipeline, hp
from ngspeciesid_amd._capi import ReadSet, NgsidError
from hp_reference import hp_reference, HpAdapter
import hp_cases as hc

pytestmark = pytest.mark.gpu


def _lists(lists):
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
    return off, np.array([p for x in lists for p in x], dtype=np.uint32)


def _all_runs(centres):
    return _lists([hp.runs(c)[0].tolist() for c in centres])


def _same(api, oracle, centres, rs, grp_off, run_off, run_start, read_order=None, k=13, w=20, clip=False, what=""):
    grp_off = np.asarray(grp_off, dtype=np.uint64)
    got = api.hp_runs(ReadSet.from_strings(centres), rs, grp_off, run_off, run_start, read_order=read_order, k=k, w=w, clip=clip)
    exp = hp_reference(oracle, centres, rs, grp_off, run_off, run_start, read_order, k, w, clip)
    assert got[1].dtype == np.int8 and np.array_equal(got[1], exp[1]), "%s: strands differ" % what
    assert got[0].dtype == np.uint32 and got[0].shape == exp[0].shape
    bad = np.nonzero((got[0] != exp[0]).reshape(len(exp[0]), -1).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d runs differ, first %d (position %d): HIP %s reference %s" % (what, len(bad), bad[0], run_start[bad[0]], got[0][bad[0]].tolist(), exp[0][bad[0]].tolist())
    return got


def _centre(rng, L, runs):
    """a centre of L bases: the runs [(start, length)] (ascending, they may touch), every other base a run of one"""
    s = []
    for a, n in sorted(runs):
        while len(s) < a: s.append(next(c for c in "ACGT"[int(rng.integers(4)):] + "ACGT" if not s or c != s[-1]))
        assert len(s) == a
        s.extend(next(c for c in "ACGT"[int(rng.integers(4)):] + "ACGT" if not s or c != s[-1]) * n)
    while len(s) < L: s.append(next(c for c in "ACGT"[int(rng.integers(4)):] + "ACGT" if c != s[-1]))
    c = "".join(s[:L])
    st, ln = hp.runs(c)
    have = dict(zip(st.tolist(), ln.tolist()))
    assert len(c) == L and all(have.get(a) == n for a, n in runs if a + n <= L)
    return c


def _vary(rng, centre, n):
    """n reads: the centre with the length of some runs changed (by -1, +1, +2), a few with a substitution as well, every second one on the minus strand; and reads
    cut so that they begin on / behind a left flank and end on / before a right flank of a run"""
    st, ln = hp.runs(centre); out = []
    for x in range(n):
        new = ln.copy()
        for j in range(len(ln)):
            if ln[j] >= 2 and rng.random() < 0.5: new[j] = max(1, ln[j] + int(rng.choice([-1, 1, 2])))
        r = list(hp.apply(centre, st, new))
        if x % 3 == 2 and len(r) > 12:
            i = int(rng.integers(len(r))); r[i] = "ACGT"[("ACGT".index(r[i]) + 1 + int(rng.integers(3))) % 4] if r[i] in "ACGT" else "A"
        out.append("".join(r))
    big = [(int(a), int(a + l)) for a, l in zip(st, ln) if l >= 2 and a >= 1 and a + l < len(centre)]
    for a, b in big[:2] + big[-2:]:
        out += [centre[a - 1:], centre[a:], centre[:b + 1], centre[:b]]
    return [hc.revcomp(r) if x % 2 else r for x, r in enumerate(out)]


def test_hand_cases_through_the_library(gpu_api, oracle):
    """tests/hp_cases.py, one group of one read each: the reference's histogram and the bucket derived by hand"""
    for clip in (False, True):
        cases = [c for c in hc.HAND if c["clip"] == clip and not c["name"].startswith("neighbours_gap_")]
        centres = [c["centre"] for c in cases]; rs = ReadSet.from_strings([c["read"] for c in cases])
        run_off, run_start = _lists([c["starts"] for c in cases])
        got = _same(gpu_api, oracle, centres, rs, np.arange(len(cases) + 1), run_off, run_start, clip=clip, what="hand cases, clip %d" % clip)
        assert (got[1] == 0).all()
        exp = np.zeros((len(run_start), 2, 17), dtype=np.uint32)
        for j, b in enumerate(b for c in cases for b in c["buckets"]):
            if b >= 0: exp[j, 0, b] = 1
        assert np.array_equal(got[0], exp)


CENTRES = {7: [(1, 3)], 8: [(1, 3), (4, 2)], 9: [(2, 3), (5, 3)],
           63: [(5, 3), (8, 2), (29, 3), (32, 3), (53, 3), (56, 4)], 64: [(5, 3), (8, 2), (29, 3), (32, 3), (56, 4), (60, 3)],
           65: [(5, 3), (8, 2), (29, 3), (32, 3), (56, 4), (61, 3)], 129: [(5, 3), (8, 2), (61, 3), (64, 3), (120, 4), (125, 3)]}


@pytest.mark.parametrize("L", sorted(CENTRES))
def test_centre_lengths(gpu_api, oracle, L):
    """nibble dword (8 positions), position store (4 positions) and row padding (64 positions) edges: runs that begin or end on a multiple of 8 and of 64, a right flank that is
    the last base of the centre; reads cut on the flanks.  Every run listed, then every second one; both clip modes; k = 4, w = 1 so that a centre of 7 bases has a strand"""
    rng = np.random.default_rng(100 + L)
    c = _centre(rng, L, CENTRES[L])
    reads = _vary(rng, c, 10)
    rs = ReadSet.from_strings(reads); grp = [0, len(reads)]
    run_off, run_start = _all_runs([c])
    got = _same(gpu_api, oracle, [c], rs, grp, run_off, run_start, k=4, w=1, what="centre of %d" % L)
    assert (got[1] == 0).sum() >= 5 and (got[1] == 1).sum() >= 5 and got[0][:, :, :16].sum() > 0
    assert got[0][0].sum() == 0 and got[0][-1].sum() == 0                                 # the first and the last run are never counted
    some = run_start[::2]
    part = _same(gpu_api, oracle, [c], rs, grp, [0, len(some)], some, k=4, w=1, clip=True, what="centre of %d, clip, every second run" % L)
    assert part[0].shape == (len(some), 2, 17)


def test_lengths_letters_and_flanks(gpu_api, oracle):
    """l = 0, 1, 14, 15, 16 and 40 on both strands, against a run of 3 and a run of 14; a foreign letter, an N, a mismatched and a deleted flank, an insertion behind the
    left flank; a run of N in the centre"""
    counts = {}
    for core in ("CAAAG", "C" + "A" * 14 + "G"):
        centre = hc.LEFT + core + hc.RIGHT
        reads = [hc.LEFT + "C" + "A" * l + "G" + hc.RIGHT for l in (0, 1, 14, 15, 16, 40)]
        reads += [hc.revcomp(r) for r in reads]
        reads += [hc.LEFT + x + hc.RIGHT for x in ("CAATAG", "CANAG", "CAAANG", "TAAAG", "CAAAT", "AAAG", "CTAAAG", "CAAAGG")]
        run_off, run_start = _all_runs([centre])
        got = _same(gpu_api, oracle, [centre], ReadSet.from_strings(reads), [0, len(reads)], run_off, run_start, what=core)
        h = got[0][run_start.tolist().index(hc.NL + 1)]
        for s in (0, 1):
            assert h[s, [0, 1, 14, 15]].tolist()[:3] == [1, 1, 1] and h[s, 15] == 3
        counts[core] = h
    assert counts["CAAAG"][0, 16] >= 6
    centre = hc.LEFT + "CNNNG" + hc.RIGHT
    run_off, run_start = _all_runs([centre])
    got = _same(gpu_api, oracle, [centre], ReadSet.from_strings([centre, hc.LEFT + "CNNG" + hc.RIGHT, hc.revcomp(centre)]), [0, 3], run_off, run_start, what="run of N")
    assert got[0][run_start.tolist().index(hc.NL + 1)].sum() == 0 and got[0].sum() > 0


@pytest.fixture(scope="module")
def groups():
    """5 groups: empty; 40 reads but no listed run; one read; 60 reads on both strands with a read that shares no minimizer (strand -1) and reads with N; empty again"""
    rng = np.random.default_rng(7)
    cs = [_centre(rng, L, [(a, 2 + (a // 20) % 5) for a in range(20, L - 20, 20)]) for L in (200, 260, 230, 300, 210)]
    reads = _vary(rng, cs[1], 32)[:40] + [cs[2][:110] + "A" + cs[2][110:]] + _vary(rng, cs[3], 52)[:60]
    assert len(reads) == 101
    reads[41 + 7] = "".join("ACGT"[int(v)] for v in rng.integers(4, size=280))
    for i, p in ((41 + 3, 60), (41 + 10, 122)):
        reads[i] = reads[i][:p] + "N" * 5 + reads[i][p + 5:]
    return cs, ReadSet.from_strings(reads), np.array([0, 0, 40, 41, 101, 101], dtype=np.uint64)


def test_strands_and_groups(gpu_api, oracle, groups):
    cs, rs, grp = groups
    lists = [hp.runs(c)[0].tolist() for c in cs]; lists[1] = []; lists[0] = lists[0][:3]
    run_off, run_start = _lists(lists)
    got = _same(gpu_api, oracle, cs, rs, grp, run_off, run_start, what="groups")
    assert got[1][41 + 7] == -1 and (got[1][41:] == 1).sum() > 20 and (got[1][41:] == 0).sum() > 20
    assert got[0][:3].sum() == 0 and got[0][int(run_off[2]):int(run_off[3])].sum() > 0 and got[0][int(run_off[2]):int(run_off[3])].max() == 1 and got[0][int(run_off[4]):].sum() == 0
    # clip = 1; a read order; only some runs; nothing listed at all
    _same(gpu_api, oracle, cs, rs, grp, run_off, run_start, clip=True, what="groups, clip")
    ro = np.arange(101, dtype=np.uint32)[::-1].copy()
    grp2 = np.array([0, 60, 61, 61, 61, 101], dtype=np.uint64)
    lists2 = [lists_[::3] for lists_ in (hp.runs(cs[3])[0].tolist(), hp.runs(cs[2])[0].tolist(), [], [], hp.runs(cs[1])[0].tolist())]
    _same(gpu_api, oracle, [cs[3], cs[2], cs[0], cs[4], cs[1]], rs, grp2, *_lists(lists2), read_order=ro, what="read order, every third run")
    z = gpu_api.hp_runs(ReadSet.from_strings(cs), rs, grp, np.zeros(6, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    assert z[0].shape == (0, 2, 17) and np.array_equal(z[1], got[1])
    z = gpu_api.hp_runs(ReadSet.from_strings(cs), rs, np.zeros(6, dtype=np.uint64), run_off, run_start)
    assert z[0].sum() == 0 and len(z[1]) == 0


def test_slice_and_tile_edges(gpu_api, oracle):
    """1 025 reads of 40 bases in one group (one more than a slice of k_hp_runs) and a centre of 300 runs (ACGT repeated: one more tile than 256 lanes)"""
    rng = np.random.default_rng(8)
    c0 = _centre(rng, 40, [(6, 3), (14, 2), (22, 4), (31, 3)])
    st, ln = hp.runs(c0); short = []
    for x in range(1025):
        new = ln.copy(); j = int(rng.integers(len(ln)))
        if ln[j] >= 2: new[j] = ln[j] + int(rng.choice([-1, 0, 1]))
        r = hp.apply(c0, st, new)
        r = (r + hc.no_repeat(rng, 2, first_not=r[-1]))[:40] if len(r) < 40 else r[:40]
        short.append(hc.revcomp(r) if x % 2 else r)
    assert all(len(r) == 40 for r in short)
    c1 = "ACGT" * 75
    s1, l1 = hp.runs(c1)
    assert len(s1) == 300
    longer = []
    for x in range(8):
        new = l1.copy(); new[rng.integers(10, 290, size=12)] = 2
        longer.append(hp.apply(c1, s1, new))
    rs = ReadSet.from_strings(short + longer)
    run_off, run_start = _all_runs([c0, c1])
    got = _same(gpu_api, oracle, [c0, c1], rs, [0, 1025, 1033], run_off, run_start, k=8, w=4, what="1 025 reads, 300 runs")
    assert (got[1][:1025] >= 0).sum() > 1000 and got[0][:int(run_off[1])].sum() > 3000 and got[0][int(run_off[1]):, :, 2].sum() > 20


@pytest.fixture(scope="module")
def bulk():
    sp = synth.make_species(3, 500, 0.15, seed=64)
    rd = synth.make_reads(sp, 2700, mu=14.0, seed=65, rc_fraction=0.5)
    rs = ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64)); species = rd["species"].numpy()
    lists = [np.nonzero(species == g)[0].astype(np.uint32) for g in range(3)]
    centres = [s.tobytes().decode() for s in sp]
    return centres, rs, _lists(lists)[0], np.concatenate(lists)


def test_chunks_give_the_same_arrays(gpu_api, bulk):
    """a budget of 1 MB holds 819 rows of a 512-position path and position matrix (64 dwords + 1 KB a row): 2 700 pairs take four chunks"""
    centres, rs, grp, ro = bulk
    cen = ReadSet.from_strings(centres); run_off, run_start = _all_runs(centres)
    gpu_api.profile_enable(True); gpu_api.profile_read()
    try:
        base = gpu_api.hp_runs(cen, rs, grp, run_off, run_start, read_order=ro)
        one = gpu_api.profile_read()[0]
        gpu_api.set_option("support_budget_mb", 1)
        try:
            again = gpu_api.hp_runs(cen, rs, grp, run_off, run_start, read_order=ro)
        finally:
            gpu_api.set_option("support_budget_mb", 0)
        many = gpu_api.profile_read()[0]
    finally:
        gpu_api.profile_enable(False)
    assert one["k_hp_runs"][0] == 1 and many["k_hp_runs"][0] >= 3 and "k_ed_align_rec" in one
    assert np.array_equal(base[0], again[0]) and np.array_equal(base[1], again[1])
    assert base[0][:, :, :16].sum() > 100000 and (base[1] == 1).sum() > 1000


def test_support_before_and_after(gpu_api, bulk):
    """the store pass with the position output between two runs without it, in one context: the support call returns what it returned"""
    centres, rs, grp, ro = bulk
    cen = ReadSet.from_strings(centres); run_off, run_start = _all_runs(centres)
    a = gpu_api.consensus_support(cen, rs, grp, read_order=ro)
    h = gpu_api.hp_runs(cen, rs, grp, run_off, run_start, read_order=ro)
    b = gpu_api.consensus_support(cen, rs, grp, read_order=ro)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[3], h[1]) and a[0].sum() > 0


def test_argument_errors(gpu_api, groups):
    cs, rs, grp = groups
    cen = ReadSet.from_strings(cs)
    st = hp.runs(cs[1])[0].tolist()
    inside = next(a for a, n in zip(*[x.tolist() for x in hp.runs(cs[1])]) if n >= 2) + 1
    for lists in ([[], [inside], [], [], []], [[], [st[5], st[2]], [], [], []], [[], [st[2], st[2]], [], [], []], [[], [len(cs[1])], [], [], []], [[], [], [], [], [0, len(cs[4])]]):
        with pytest.raises(NgsidError) as ex:
            gpu_api.hp_runs(cen, rs, grp, *_lists(lists))
        assert ex.value.code == -2
    ok = gpu_api.hp_runs(cen, rs, grp, *_lists([[], [st[-1]], [], [0], []]))
    assert ok[0].shape == (2, 2, 17)


# ---- pipeline and command line
LAX = dict(min_depth=4, min_share=0.3, min_margin=0.0, min_strand_depth=1000)          # thresholds that let the vote change runs of a noisy 60-read cluster: the layers are under test, not the policy


@pytest.fixture(scope="module")
def two_clusters(oracle):
    """2 templates of 400 bases with six planted runs of 5 - 7 bases each, 120 reads at mu = 14 on both strands, every run of at least 4 bases of a read shortened by one
    with probability 0.3; in score order, as the pipeline takes them"""
    from ngspeciesid_amd.hostutil import subset_reads
    from ngspeciesid_amd.ptable import select_p_table
    rng = np.random.default_rng(5)
    sp = synth.make_species(2, 400, 0.25, seed=5)
    T = [hc.with_runs(s.tobytes().decode(), [(40 + 60 * i, "ACGT"[(i + g) % 4], 5 + i % 3) for i in range(6)]) for g, s in enumerate(sp)]
    rd = synth.make_reads([np.frombuffer(t.encode(), dtype=np.uint8).copy() for t in T], 120, mu=14.0, seed=6, rc_fraction=0.5)
    rs = hc.bias_reads(ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64)), rng, 0.3)
    score, err, keep = oracle.score_reads(rs, 13, 7.0)
    idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
    sub = subset_reads(rs, idx)
    return T, rs, sub, score[idx], dict(k=13, w=20, abundance_ratio=0.05, racon_iter=2, band=0, p_shared=select_p_table(13, 20), acc_rank=np.arange(sub.n, dtype=np.uint32))


def _same_changes(xs, ys):
    assert len(xs) == len(ys)
    for x, y in zip(xs, ys):
        assert len(x) == len(y)
        for c, d in zip(x, y):
            assert sorted(c) == sorted(d) == ["hist", "letter", "new", "old", "pos", "round"]
            assert all(c[key] == d[key] for key in c if key != "hist") and np.array_equal(c["hist"], d["hist"]) and c["hist"].dtype == d["hist"].dtype == np.uint32


def test_pipeline_through_hip_equals_the_adapter(gpu_api, oracle, two_clusters):
    T, _, sub, score, kw = two_clusters
    a = pipeline.run_hot_path(gpu_api, sub, score, hp_polish=True, hp_kwargs=LAX, support=True, **kw)
    b = pipeline.run_hot_path(HpAdapter(oracle), sub, score, hp_polish=True, hp_kwargs=LAX, **kw)
    assert a["centers"] == b["centers"] and len(a["centers"]) == len(a["hp_polish"]) == 2
    _same_changes(a["hp_polish"], b["hp_polish"])
    assert sum(len(ch) for ch in a["hp_polish"]) >= 1
    plain = pipeline.run_hot_path(gpu_api, sub, score, **kw)
    assert sorted(plain) == sorted(k for k in a if k not in ("hp_polish", "support")) and np.array_equal(plain["rep_of"], a["rep_of"])
    for c, p, ch, sup in zip(a["centers"], plain["centers"], a["hp_polish"], a["support"]):
        assert c[:3] == p[:3] and c[4] == p[4] and len(sup) == len(c[3])                           # the support is that of the corrected sequence
        seq = p[3]
        for rnd in sorted({x["round"] for x in ch}):
            part = [x for x in ch if x["round"] == rnd]
            assert all(seq[x["pos"]] == x["letter"] and 1 <= x["new"] <= 14 and x["new"] != x["old"] for x in part)
            seq = hp.apply(seq, [x["pos"] for x in part], [x["new"] for x in part])
        assert seq == c[3] and (c[3] == p[3]) == (len(ch) == 0)
    # the default thresholds through the same path, and the multi-sample driver with the two clusters as one sample
    d = pipeline.run_hot_path(gpu_api, sub, score, hp_polish=True, **kw)
    e = pipeline.run_hot_path_samples(gpu_api, sub, score, [0, sub.n], hp_polish=True, **kw)
    assert len(e) == 1 and e[0]["centers"] == d["centers"]
    _same_changes(e[0]["hp_polish"], d["hp_polish"])


def _files(out):
    res = {}
    for root, _, fs in os.walk(out):
        for f in fs:
            res[os.path.relpath(os.path.join(root, f), out)] = open(os.path.join(root, f), "rb").read()
    return res


def test_cli_flag(gpu_api, tmp_path, two_clusters):
    """--hp_polish: hp_polish.tsv, and the consensus files carry the sequence the table describes; every other file is what the run without the flag writes"""
    from ngspeciesid_amd import cli as _cli, fastpath
    T, rs, _, _, _ = two_clusters
    fq = str(tmp_path / "in.fastq")
    with open(fq, "w") as f:
        for i in range(rs.n):
            s, q = rs.get(i)
            f.write("@r%d\n%s\n+\n%s\n" % (i, s, q))
    lax = ["--hp_min_depth", "4", "--hp_min_share", "0.3", "--hp_min_margin", "0", "--hp_min_strand_depth", "1000"]
    res = []
    for flag in ([], ["--hp_polish"] + lax):
        out = str(tmp_path / ("o%d" % len(flag))); os.makedirs(out)
        args = _cli.build_parser().parse_args(["--ont", "--fastq", fq, "--outfolder", out, "--t", "1", "--consensus", "--racon", "--racon_iter", "2", "--abundance_ratio", "0.05"] + flag); args.k, args.w = 13, 20
        fastpath.main(args, api=gpu_api)
        res.append(_files(out))
    a, b = res
    assert sorted(set(b) - set(a)) == ["hp_polish.tsv"] and set(a) <= set(b)
    rows = [r.split("\t") for r in b["hp_polish.tsv"].decode().splitlines()]
    assert rows[0] == ["cluster_id", "pos", "letter", "old_len", "new_len", "round", "hist_plus", "hist_minus"] and len(rows) >= 2
    assert all(len(r) == 8 and len(r[6].split(",")) == len(r[7].split(",")) == 17 for r in rows[1:])
    changed = {os.path.join("racon_cl_id_" + r[0], "consensus.fasta") for r in rows[1:]}
    assert all(a[f] == b[f] for f in a if f not in changed and f != "logfile.txt") and all(a[f] != b[f] for f in changed)
    for fa in changed:
        cid = fa.split(os.sep)[0][len("racon_cl_id_"):]
        head0, seq = a[fa].decode().split("\n")[:2]; head1, seq1 = b[fa].decode().split("\n")[:2]
        mine = [r for r in rows[1:] if r[0] == cid]
        for rnd in sorted({int(r[5]) for r in mine}):
            part = [r for r in mine if int(r[5]) == rnd]
            assert all(seq[int(r[1])] == r[2] for r in part)
            seq = hp.apply(seq, [int(r[1]) for r in part], [int(r[4]) for r in part])
        assert seq == seq1 and " LN:i:%d " % len(seq1) in head1 and head0.split(" ")[0] == head1.split(" ")[0]
    # --medaka stays refused, with and without the pass
    with pytest.raises(SystemExit):
        _cli.cli(["--ont", "--fastq", fq, "--outfolder", str(tmp_path / "m"), "--consensus", "--medaka", "--hp_polish"])


def test_cli_flag_under_fastq_dir(gpu_api, tmp_path, two_clusters):
    """--fastq_dir: one hp_polish.tsv per sample folder - the table a run of that file alone writes - and hp_polish_all.tsv with the sample in front"""
    from ngspeciesid_amd import cli as _cli, fastpath
    T, rs, _, _, _ = two_clusters
    os.makedirs(str(tmp_path / "in"))
    for name, n in (("s1", rs.n), ("s2", rs.n - 7)):
        with open(str(tmp_path / "in" / (name + ".fastq")), "w") as f:
            for i in range(n):
                s, q = rs.get(i)
                f.write("@r%d\n%s\n+\n%s\n" % (i, s, q))
    common = ["--ont", "--t", "1", "--consensus", "--racon", "--racon_iter", "2", "--abundance_ratio", "0.05", "--hp_polish", "--hp_min_depth", "4", "--hp_min_share", "0.3",
              "--hp_min_margin", "0", "--hp_min_strand_depth", "1000"]
    outs = {}
    for key, src in (("dir", ["--fastq_dir", str(tmp_path / "in")]), ("s1", ["--fastq", str(tmp_path / "in" / "s1.fastq")]), ("s2", ["--fastq", str(tmp_path / "in" / "s2.fastq")])):
        out = str(tmp_path / ("o_" + key)); os.makedirs(out)
        args = _cli.build_parser().parse_args(src + ["--outfolder", out] + common); args.k, args.w = 13, 20
        fastpath.main(args, api=gpu_api)
        outs[key] = _files(out)
    rows = []
    for s in ("s1", "s2"):
        tab = outs["dir"][os.path.join(s, "hp_polish.tsv")]
        assert tab == outs[s]["hp_polish.tsv"] and len(tab.decode().splitlines()) >= 2
        rows += [s + "\t" + r for r in tab.decode().splitlines()[1:]]
        for f in outs[s]:
            if f.endswith("consensus.fasta"): assert outs["dir"][os.path.join(s, f)] == outs[s][f]
    allt = outs["dir"]["hp_polish_all.tsv"].decode().splitlines()
    assert allt[0].split("\t")[:2] == ["sample", "cluster_id"] and allt[1:] == rows
