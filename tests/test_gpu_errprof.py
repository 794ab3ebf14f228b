"""GPU: ngsid_error_profile (include/ngsid_errprof.h) through the C-ABI == its definition restated from the oracle's parts (tests/errprof_reference.py), array for array -
counts, qtab and strand -, the hand tables of tests/errprof_cases.py, the header's identities against Api.consensus_support and Api.read_cigars, and the pipeline / CLI
layers on top of it.  The shapes are small on purpose: every case is an edge of the path matrix, of a 64-position step or of the kernel's slices."""
import os
import ctypes as C
import numpy as np
import pytest
from oracle_lib import GOLD
from ngspeciesid_amd import synth, pipeline, errprof, fastio
from ngspeciesid_amd._capi import ReadSet, NgsidError, SupportParams, _p
from ngspeciesid_amd.hostutil import subset_reads
from ngspeciesid_amd.ptable import select_p_table
from errprof_reference import errprof_reference, check_identities, NCOUNT, NQ, PAIR, INS_LETTER, CEN_OTHER, READS, INS_LEN, DEL_LEN, HPCTX
import errprof_cases as ec
import hp_cases as hc

pytestmark = pytest.mark.gpu
SLICE = 1024                                                                    # EP_SLICE of csrc/k_errprof.hip: pairs per workgroup


def _names(t):
    return {int(i): int(t[i]) for i in np.nonzero(t)[0]}


def _same(api, oracle, centres, rs, grp_off, read_order=None, k=13, w=20, clip=False, what="", got=None):
    grp_off = np.asarray(grp_off, dtype=np.uint64)
    if got is None: got = api.error_profile(ReadSet.from_strings(centres), rs, grp_off, read_order=read_order, k=k, w=w, clip=clip)
    exp = errprof_reference(oracle, centres, rs, grp_off, read_order, k, w, clip)
    assert got[2].dtype == np.int8 and np.array_equal(got[2], exp[2]), what + ": strand"
    assert got[0].dtype == np.uint64 and got[0].shape == exp[0].shape == (len(centres), 2, NCOUNT) and got[1].dtype == np.uint64 and got[1].shape == exp[1].shape == (len(centres), 2, NQ, 3)
    for g in range(len(centres)):
        for s in (0, 1):
            assert np.array_equal(got[0][g, s], exp[0][g, s]), "%s: counts of group %d, strand %d: HIP %s reference %s" % (what, g, s, _names(got[0][g, s]), _names(exp[0][g, s]))
            assert np.array_equal(got[1][g, s], exp[1][g, s]), "%s: qtab of group %d, strand %d: HIP %s reference %s" % (what, g, s, _names(got[1][g, s].ravel()), _names(exp[1][g, s].ravel()))
    return got


def _quals(rng, reads, lo=35, hi=90):
    return ["".join(chr(int(v)) for v in rng.integers(lo, hi, size=len(r))) for r in reads]


@pytest.mark.parametrize("clip", [False, True])
def test_hand_cases_through_the_library(gpu_api, oracle, clip):
    centres, reads, quals, grp_off, strand = ec.hand_sets()
    rs = ReadSet.from_strings(reads, quals)
    got = _same(gpu_api, oracle, centres, rs, grp_off, clip=clip, what="hand cases, clip %d" % clip)
    exp_c, exp_q = ec.hand_expected(clip)
    assert got[2].tolist() == strand
    for g, c in enumerate(ec.HAND):
        assert np.array_equal(got[0][g], exp_c[g]) and np.array_equal(got[1][g], exp_q[g]), c["name"]
    if clip: return
    # nothing listed at all, no reads at all, a centre of length 0, no group at all
    cen = ReadSet.from_strings(centres)
    z = gpu_api.error_profile(cen, rs, np.zeros(len(centres) + 1, dtype=np.uint64))
    assert z[0].shape == (len(centres), 2, NCOUNT) and z[0].sum() == 0 and z[1].sum() == 0 and len(z[2]) == 0
    z = gpu_api.error_profile(cen, ReadSet.from_strings([]), np.zeros(len(centres) + 1, dtype=np.uint64))
    assert z[0].sum() == 0 and z[1].sum() == 0
    z = gpu_api.error_profile(ReadSet.from_strings(["", centres[0]]), rs, np.array([0, 1, 2], dtype=np.uint64), read_order=np.array([1, 0], dtype=np.uint32))
    assert z[0][0].sum() == 0 and np.array_equal(z[0][1], exp_c[0]) and np.array_equal(z[1][1], exp_q[0]) and z[2].tolist() == [-1, 0]
    z = gpu_api.error_profile(ReadSet.from_strings([]), rs, np.zeros(1, dtype=np.uint64))
    assert z[0].shape == (0, 2, NCOUNT) and z[1].shape == (0, 2, NQ, 3)


def _centre_with_runs(rng, L):
    s = []
    while len(s) < L:
        c = "ACGT"[int(rng.integers(4))]
        if s and c == s[-1]: continue
        s += [c] * (int(rng.integers(2, 5)) if rng.random() < 0.15 else 1)
    return "".join(s[:L])


def _ins(rng, n, left, right):
    """n letters, no two neighbours equal, that begin with another letter than `left` and end with another than `right`"""
    while True:
        s = hc.no_repeat(rng, n, first_not=left)
        if s[-1] != right: return s


def _avoid(rng, n, letter):
    """n letters without `letter`, no two neighbours equal.  The traceback takes a diagonal step wherever it may: a gap stays ONE run of its full length only when the
    letter in front of it does not occur among the letters it skips"""
    out = []
    while len(out) < n:
        c = "ACGT"[int(rng.integers(4))]
        if c != letter and (not out or c != out[-1]): out.append(c)
    return "".join(out)


@pytest.mark.parametrize("L", [7, 8, 9, 63, 64, 65, 129, 200])
def test_centre_lengths_across_steps(gpu_api, oracle, L):
    """nibble dword (8 positions), 64-position step and row stride edges; k = 4, w = 1 so that a centre of 7 bases has a strand.  Ten and more reads on both strands: the
    centre itself, 'D' runs over 63 | 64 and 127 | 128 and up to 63, 'I' runs behind 63 and 64, gaps in front of the last base, an N, a substitution, cut reads"""
    rng = np.random.default_rng(700 + L)
    c = _centre_with_runs(rng, L)
    reads = [c, c[:L // 2] + "N" + c[L // 2 + 1:], c[1:], c[:-1], c[:L - 1] + _ins(rng, 2, c[L - 2], c[L - 1]) + c[L - 1:], c[:max(1, L - 3)] + c[L - 1:],
             c[:L // 3] + "ACGT"[("ACGT".index(c[L // 3]) + 1) % 4] + c[L // 3 + 1:], "GATTA" + c + "CCTG", c[:2] + c[3:], c[:3] + _ins(rng, 1, c[2], c[3]) + c[3:]]
    if L > 70:
        reads += [c[:62] + c[66:], c[:60] + c[64:], c[:64] + c[66:], c[:64] + _ins(rng, 3, c[63], c[64]) + c[64:], c[:65] + _ins(rng, 2, c[64], c[65]) + c[65:], c[:63] + _avoid(rng, 17, c[62]) + c[63:]]
    if L > 140:
        reads += [c[:126] + c[130:], c[:120] + c[128:], c[:128] + _ins(rng, 1, c[127], c[128]) + c[128:], c[:50] + c[135:]]
    reads = [hc.revcomp(r) if x % 2 else r for x, r in enumerate(reads)] + [hc.revcomp(r) if not x % 2 else r for x, r in enumerate(reads)]
    rs = ReadSet.from_strings(reads, _quals(rng, reads))
    for clip in (False, True):
        got = _same(gpu_api, oracle, [c], rs, [0, len(reads)], k=4, w=1, clip=clip, what="centre of %d, clip %d" % (L, clip))
    nc = _same(gpu_api, oracle, [c], rs, [0, len(reads)], k=4, w=1, what="centre of %d" % L)
    assert (nc[2] == 0).sum() >= 5 and (nc[2] == 1).sum() >= 5 and nc[0][0, :, READS].sum() >= 10
    if L > 70: assert nc[0][0, :, DEL_LEN:DEL_LEN + 16].sum() >= 6 and nc[0][0, :, INS_LEN:INS_LEN + 16].sum() >= 6 and nc[0][0, :, INS_LEN + 15].sum() >= 2


def test_length_buckets_and_letters(gpu_api, oracle):
    """'I' and 'D' runs of 1, 15, 16, 17 and 40 on both strands against centre runs of 7, 8, 9 and 14 (the 16+ and 8+ buckets); N in reads, a run of N in the centre;
    the quality bytes 33 and 126, and 20, which lies below the scale and counts as quality 0"""
    rng = np.random.default_rng(41)
    mid = hc.no_repeat(rng, 10, first_not=hc.RIGHT[-1]); zone = _avoid(rng, 40, mid[-1]); tail = hc.no_repeat(rng, 60, first_not=zone[-1])
    post = mid + zone + tail                                                     # the gaps begin behind mid: none of the 40 letters a 'D' run skips is mid's last, and anchors longer than the gap on both sides
    centres, reads, off = [], [], [0]
    for r in (7, 8, 9, 14):
        c = hc.LEFT + "C" + "A" * r + "T" + hc.RIGHT + post
        p = len(c) - 100
        centres.append(c)
        rd = [c, c[:42] + "A" + c[42:], c[:43] + c[44:], c[:41] + "N" + c[42:]]                                            # the run one longer, one shorter, an N for its first base
        for l in (1, 15, 16, 17, 40):
            rd += [c[:p] + c[p + l:], c[:p] + _avoid(rng, l, c[p - 1]) + c[p:]]
        reads += rd + [hc.revcomp(x) for x in rd]
        off.append(len(reads))
    centres.append(hc.LEFT + "CNNNT" + hc.RIGHT + post)
    reads += [centres[-1], hc.LEFT + "CNNT" + hc.RIGHT + post, hc.LEFT + "CAGAT" + hc.RIGHT + post, hc.revcomp(hc.LEFT + "CT" + hc.RIGHT + post)]
    off.append(len(reads))
    quals = _quals(rng, reads)
    quals[0] = chr(33) * 5 + chr(126) * 5 + chr(20) * 5 + quals[0][15:]
    quals[1] = chr(126) * len(reads[1]); quals[2] = chr(20) * 40 + chr(33) * (len(reads[2]) - 40)
    rs = ReadSet(np.frombuffer("".join(reads).encode(), dtype=np.uint8), np.frombuffer("".join(quals).encode("latin-1"), dtype=np.uint8),
                 np.concatenate(([0], np.cumsum([len(r) for r in reads]))).astype(np.uint64))
    got = _same(gpu_api, oracle, centres, rs, off, what="length buckets")
    c = got[0].sum(axis=1)
    for g, r in enumerate((7, 8, 9, 14)):
        assert c[g, HPCTX + (min(r, 8) - 1) * 4] > 20 * r * 0.9 and c[g, INS_LEN + 15] >= 4 and c[g, DEL_LEN + 15] >= 4 and c[g, INS_LEN + 14] >= 2 and c[g, DEL_LEN + 14] >= 2
    assert c[4, CEN_OTHER] >= 3 and c[:4, PAIR + 4].sum() >= 8 and got[1][0, 0, 0].sum() >= 10 and got[1][0, 0, 93].sum() >= 5 + len(reads[1]) - 2
    _same(gpu_api, oracle, centres, rs, off, clip=True, what="length buckets, clip")


@pytest.fixture(scope="module")
def groups():
    """5 groups: empty; 40 reads; one read; 60 reads on both strands with a read that shares no minimizer (strand -1) and reads with N; empty again"""
    rng = np.random.default_rng(7)
    sp = synth.make_species(5, 240, 0.3, seed=77)
    cs = [s.tobytes().decode() for s in sp]
    rd = synth.make_reads([sp[1], sp[3]], 150, mu=13.0, seed=78, rc_fraction=0.5)
    rs = ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64)); which = rd["species"].numpy()
    a = np.nonzero(which == 0)[0][:40]; b = np.nonzero(which == 1)[0][:60]
    assert len(a) == 40 and len(b) == 60
    reads = [rs.get(int(i)) for i in a] + [(cs[2][:110] + "A" + cs[2][110:], "5" * (len(cs[2]) + 1))] + [rs.get(int(i)) for i in b]
    reads[41 + 7] = ("".join("ACGT"[int(v)] for v in rng.integers(4, size=230)), "I" * 230)
    for i, p in ((41 + 3, 60), (41 + 10, 122)):
        s, q = reads[i]; reads[i] = (s[:p] + "N" * 5 + s[p + 5:], q)
    return cs, ReadSet.from_strings([r[0] for r in reads], [r[1] for r in reads]), np.array([0, 0, 40, 41, 101, 101], dtype=np.uint64)


def test_strands_and_groups(gpu_api, oracle, groups):
    cs, rs, grp = groups
    got = _same(gpu_api, oracle, cs, rs, grp, what="groups")
    assert got[2][41 + 7] == -1 and (got[2][41:] == 1).sum() > 15 and (got[2][41:] == 0).sum() > 15
    assert got[0][0].sum() == 0 and got[0][4].sum() == 0 and got[0][2, :, READS].tolist() == [1, 0] and got[0][2, 0, INS_LEN] == 1 and got[0][3, :, PAIR + 4].sum() >= 5
    _same(gpu_api, oracle, cs, rs, grp, clip=True, what="groups, clip")
    # a read order
    ro = np.arange(101, dtype=np.uint32)[::-1].copy()
    grp2 = np.array([0, 60, 61, 61, 61, 101], dtype=np.uint64)
    perm = _same(gpu_api, oracle, [cs[3], cs[2], cs[0], cs[4], cs[1]], rs, grp2, read_order=ro, what="read order")
    assert np.array_equal(perm[0][0], got[0][3]) and np.array_equal(perm[1][4], got[1][1]) and np.array_equal(perm[2], got[2][::-1])
    # FASTA reads: the same counts, an all-zero qtab; qualities=False: no table, the same counts
    fa = gpu_api.error_profile(ReadSet.from_strings(cs), ReadSet(rs.seq, None, rs.off), grp)
    assert np.array_equal(fa[0], got[0]) and fa[1].shape == got[1].shape and fa[1].sum() == 0 and np.array_equal(fa[2], got[2])
    nq = gpu_api.error_profile(ReadSet.from_strings(cs), rs, grp, qualities=False)
    assert nq[1] is None and np.array_equal(nq[0], got[0]) and np.array_equal(nq[2], got[2])
    # a device-resident read set
    dev = gpu_api.upload_reads(rs)
    try:
        on = gpu_api.error_profile(ReadSet.from_strings(cs), dev, grp)
    finally:
        dev.release()
    assert all(np.array_equal(x, y) for x, y in zip(on, got))


def test_one_more_pair_than_a_slice(gpu_api, oracle):
    """SLICE + 1 reads of about 40 bases in one group, and a second group behind it"""
    rng = np.random.default_rng(8)
    c0 = _centre_with_runs(rng, 40); c1 = _centre_with_runs(rng, 50)
    reads = []
    for x in range(SLICE + 1 + 9):
        c = c0 if x <= SLICE else c1
        r = list(c)
        i = int(rng.integers(4, len(r) - 4)); kind = x % 4
        if kind == 1: r[i] = "ACGT"[("ACGT".index(r[i]) + 1) % 4]
        elif kind == 2: del r[i]
        elif kind == 3: r.insert(i, "ACGT"[int(rng.integers(4))])
        r = "".join(r)
        reads.append(hc.revcomp(r) if x % 2 else r)
    rs = ReadSet.from_strings(reads, _quals(rng, reads))
    got = _same(gpu_api, oracle, [c0, c1], rs, [0, SLICE + 1, SLICE + 10], k=8, w=4, what="one more pair than a slice")
    assert got[0][0, :, READS].sum() > SLICE - 20 and got[0][1, :, READS].sum() >= 7


@pytest.mark.parametrize("clip", [False, True])
def test_random_groups(gpu_api, oracle, clip):
    """2 groups x 200 reads of about 300 letters at mu = 14 and 9, both strands, read_order permuted"""
    sp = synth.make_species(2, 300, 0.2, seed=91)
    rd = [synth.make_reads(sp, 250, mu=mu, seed=92 + i, rc_fraction=0.5) for i, mu in enumerate((14.0, 9.0))]
    parts = [ReadSet(r["seq"].numpy(), r["qual"].numpy(), r["off"].numpy().astype(np.uint64)) for r in rd]
    species = np.concatenate([r["species"].numpy() for r in rd])
    lens = np.concatenate([np.diff(p.off.astype(np.int64)) for p in parts])
    o = np.zeros(len(lens) + 1, dtype=np.uint64); o[1:] = np.cumsum(lens)
    rs = ReadSet(np.concatenate([p.seq for p in parts]), np.concatenate([p.qual for p in parts]), o)
    rng = np.random.default_rng(3)
    lists = [rng.permutation(np.nonzero(species == g)[0])[:200].astype(np.uint32) for g in range(2)]
    assert all(len(l) == 200 for l in lists)
    got = _same(gpu_api, oracle, [s.tobytes().decode() for s in sp], rs, [0, 200, 400], np.concatenate(lists), clip=clip, what="random groups, clip %d" % clip)
    assert (got[2] == 1).sum() > 100 and (got[2] == 0).sum() > 100 and got[0][:, :, INS_LEN:INS_LEN + 16].sum() > 500 and got[0][:, :, DEL_LEN + 1:DEL_LEN + 16].sum() > 20


@pytest.fixture(scope="module")
def bulk():
    sp = synth.make_species(3, 500, 0.15, seed=64)
    rd = synth.make_reads(sp, 2700, mu=14.0, seed=65, rc_fraction=0.5)
    rs = ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64)); species = rd["species"].numpy()
    lists = [np.nonzero(species == g)[0].astype(np.uint32) for g in range(3)]
    centres = [s.tobytes().decode() for s in sp]
    return centres, rs, np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64), np.concatenate(lists)


def test_chunks_give_the_same_arrays(gpu_api, bulk):
    """a budget of 1 MB holds 819 rows of a 512-position path and position matrix (64 dwords + 1 KB a row): 2 700 pairs take four chunks"""
    centres, rs, grp, ro = bulk
    cen = ReadSet.from_strings(centres)
    gpu_api.profile_enable(True); gpu_api.profile_read()
    try:
        base = gpu_api.error_profile(cen, rs, grp, read_order=ro)
        one = gpu_api.profile_read()[0]
        gpu_api.set_option("support_budget_mb", 1)
        try:
            again = gpu_api.error_profile(cen, rs, grp, read_order=ro)
        finally:
            gpu_api.set_option("support_budget_mb", 0)
        many = gpu_api.profile_read()[0]
    finally:
        gpu_api.profile_enable(False)
    assert one["k_errprof"][0] == 1 and many["k_errprof"][0] >= 3 and "k_ed_align_rec" in one
    assert all(np.array_equal(x, y) for x, y in zip(base, again))
    assert base[0][:, :, PAIR:PAIR + 24].sum() > 1000000 and (base[2] == 1).sum() > 1000 and base[1].sum() > 1000000


@pytest.mark.parametrize("clip", [False, True])
def test_identities_on_the_device(gpu_api, bulk, clip):
    centres, rs, grp, ro = bulk
    cen = ReadSet.from_strings(centres)
    counts, qtab, strand = gpu_api.error_profile(cen, rs, grp, read_order=ro, clip=clip)
    sup, cen_off, used, st2 = gpu_api.consensus_support(cen, rs, grp, read_order=ro, clip=clip)
    aln, _, _, st3 = gpu_api.read_cigars(cen, rs, grp, read_order=ro, clip=clip)
    assert np.array_equal(strand, st2) and np.array_equal(strand, st3)
    check_identities(counts, qtab, sup, cen_off, used, aln, grp)


def test_support_before_and_after(gpu_api, bulk):
    """the call that reads the oriented qualities between two support calls in one context: the support call returns what it returned"""
    centres, rs, grp, ro = bulk
    cen = ReadSet.from_strings(centres)
    a = gpu_api.consensus_support(cen, rs, grp, read_order=ro)
    e = gpu_api.error_profile(cen, rs, grp, read_order=ro)
    b = gpu_api.consensus_support(cen, rs, grp, read_order=ro)
    no_q = gpu_api.consensus_support(cen, ReadSet(rs.seq, None, rs.off), grp, read_order=ro)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and all(np.array_equal(x, y) for x, y in zip(a, no_q)) and np.array_equal(a[3], e[2]) and a[0].sum() > 0


def test_argument_errors(gpu_api, groups):
    cs, rs, grp = groups
    cen = ReadSet.from_strings(cs)
    counts = np.zeros((5, 2, NCOUNT), dtype=np.uint64)
    call = lambda prm, cnt, ro=None: gpu_api._call("error_profile", C.byref(cen.c), C.byref(rs.c), _p(ro), _p(grp), C.c_uint64(5), C.byref(prm), _p(cnt), None, None)
    assert call(SupportParams(13, 20, 0), counts) == 0 and counts.sum() > 0
    assert call(SupportParams(13, 20, 0), None) == -2                                # null counts
    assert call(SupportParams(13, 20, 2), counts) == -2                              # clip is 0 or 1
    twice = np.arange(101, dtype=np.uint32); twice[50] = 3                            # read 3 under group 1 and under group 3
    assert call(SupportParams(13, 20, 0), counts, twice) == -2
    with pytest.raises(NgsidError) as ex:
        gpu_api.error_profile(cen, rs, grp, read_order=twice)
    assert ex.value.code == -2
    with pytest.raises(ValueError):
        gpu_api.error_profile(gpu_api.upload_reads(cen), rs, grp)


# ---- pipeline and command line
def _sample_h1(api):
    rd = fastio.read_fastq(os.path.join(GOLD, "sample_h1.fastq"))
    rs = rd[1] if isinstance(rd, tuple) else rd
    score, err, keep = api.score_reads(rs, 13, 7.0)
    idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
    return subset_reads(rs, idx), score[idx]


KW = dict(k=13, w=20, abundance_ratio=0.05, racon_iter=2, band=0, p_shared=select_p_table(13, 20))


def _same_parts(xs, ys):
    assert len(xs) == len(ys)
    for x, y in zip(xs, ys):
        assert sorted(x) == sorted(y) == ["counts", "n_listed", "n_stranded", "qtab"]
        assert np.array_equal(x["counts"], y["counts"]) and np.array_equal(x["qtab"], y["qtab"]) and (x["n_listed"], x["n_stranded"]) == (y["n_listed"], y["n_stranded"])


def test_pipeline_key(gpu_api, oracle):
    sub, score = _sample_h1(gpu_api)
    kw = dict(KW, acc_rank=np.arange(sub.n, dtype=np.uint32))
    a = pipeline.run_hot_path(gpu_api, sub, score, **kw)
    b = pipeline.run_hot_path(gpu_api, sub, score, error_profile=True, **kw)
    assert sorted(b) == sorted(list(a) + ["error_profile"]) and a["centers"] == b["centers"] and np.array_equal(a["rep_of"], b["rep_of"])
    for key in a:
        if key != "centers": assert np.array_equal(a[key], b[key]), key
    lists = [np.concatenate([np.nonzero(b["rep_of"] == r)[0] for r in c[4]]).astype(np.uint32) for c in b["centers"]]      # the pooled lists
    centres = [c[3] for c in b["centers"]]
    assert centres and len(b["error_profile"]) == len(centres)
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
    got = _same(gpu_api, oracle, centres, sub, off, np.concatenate(lists), what="sample_h1")
    for g, e in enumerate(b["error_profile"]):
        assert np.array_equal(e["counts"], got[0][g]) and np.array_equal(e["qtab"], got[1][g]) and e["n_listed"] == len(lists[g]) and e["n_stranded"] == int((got[2][int(off[g]):int(off[g + 1])] >= 0).sum())
    assert got[0][:, :, READS].sum() > 200 and errprof.rates(got[0])["both"]["total"] > 0.01
    # many samples in one pass: the key of every sample is what the sample gets alone
    half = sub.n // 2
    many = pipeline.run_hot_path_samples(gpu_api, sub, score, np.array([0, half, sub.n], dtype=np.uint64), error_profile=True, **kw)
    assert len(many) == 2
    for s, (lo, hi) in enumerate(((0, half), (half, sub.n))):
        part = subset_reads(sub, np.arange(lo, hi))
        alone = pipeline.run_hot_path(gpu_api, part, score[lo:hi], error_profile=True, **dict(kw, acc_rank=np.arange(hi - lo, dtype=np.uint32)))
        assert many[s]["centers"] == alone["centers"] and len(alone["centers"]) >= 1
        _same_parts(many[s]["error_profile"], alone["error_profile"])
    no_q = pipeline.run_hot_path(gpu_api, sub, score, error_profile=True, error_profile_kwargs=dict(qualities=False), **kw)
    assert all(e["qtab"] is None and np.array_equal(e["counts"], f["counts"]) for e, f in zip(no_q["error_profile"], b["error_profile"]))


def _files(out):
    res = {}
    for root, _, fs in os.walk(out):
        for f in fs:
            res[os.path.relpath(os.path.join(root, f), out)] = open(os.path.join(root, f), "rb").read()
    return res


def _run(api, tmp, name, src, flags):
    from ngspeciesid_amd import cli as _cli, fastpath
    out = str(tmp / name); os.makedirs(out)
    args = _cli.build_parser().parse_args(["--ont"] + src + ["--outfolder", out, "--t", "1", "--consensus", "--racon", "--racon_iter", "1"] + flags); args.k, args.w = 13, 20
    fastpath.main(args, api=api)
    return out, _files(out)


def test_cli_flag_and_sub_command(gpu_api, tmp_path):
    from ngspeciesid_amd import cli as _cli, recruit, sam
    fq = os.path.join(GOLD, "sample_h1.fastq")
    _, a = _run(gpu_api, tmp_path, "plain", ["--fastq", fq], [])
    out, b = _run(gpu_api, tmp_path, "flag", ["--fastq", fq], ["--error_profile"])
    assert sorted(set(b) - set(a)) == ["error_profile.tsv", "quality_calibration.tsv"] and all(a[f] == b[f] for f in a if f != "logfile.txt")
    tab = errprof.read_table(os.path.join(out, "error_profile.tsv"))
    stems = sorted(f.split(os.sep)[0][len("racon_cl_id_"):] for f in a if f.endswith(os.sep + "consensus.fasta"))
    assert stems and sorted(tab["counts"]) == sorted(stems) and all(0.0 < tab["rates"][s]["both"]["total"] < 0.3 for s in stems)
    assert all(tab["rates"][s]["both"] == errprof.rates(tab["counts"][s])["both"] for s in stems)
    cal = errprof.read_calibration(os.path.join(out, "quality_calibration.tsv"))
    assert len(cal["q"]) >= 5 and (np.diff(cal["q"]) > 0).all() and ((cal["n_match"] + cal["n_sub"] + cal["n_ins"]).astype(np.int64) >= errprof.MIN_OBS).all()
    # the sub-command: the sorted reads against the consensuses the run wrote - its table is Api.error_profile on the recruited lists
    fa = str(tmp_path / "cons.fasta")
    with open(fa, "w") as f:
        for s in stems: f.write(b[os.path.join("racon_cl_id_" + s, "consensus.fasta")].decode())
    sq = os.path.join(out, "sorted.fastq")
    sargs = _cli._errprof_subparser(__import__("argparse").ArgumentParser()).parse_args(["--fastq", sq, "--fasta", fa, "--outfolder", str(tmp_path / "ep")])
    res = errprof.errprof_fastq(sargs, api=gpu_api)
    names, rs, _ = fastio.read_fastq(sq)
    seqs = [b[os.path.join("racon_cl_id_" + s, "consensus.fasta")].decode().split("\n")[1] for s in stems]
    rec = recruit.run(gpu_api, rs, [0, rs.n], [seqs])[0]
    lists = sam.recruited_lists(rec["hits"], rec["status"], len(seqs))[0]
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
    counts, qtab, _ = gpu_api.error_profile(ReadSet.from_strings(seqs), rs, off, read_order=np.concatenate(lists).astype(np.uint32))
    sub = errprof.read_table(str(tmp_path / "ep" / "error_profile.tsv"))
    assert len(sub["counts"]) == len(stems) and sum(len(l) for l in lists) > 100
    for g, p in enumerate(res["parts"]):
        assert np.array_equal(p["counts"], counts[g]) and np.array_equal(p["qtab"], qtab[g]) and np.array_equal(sub["counts"][res["ids"][g]], counts[g])
    # --error_profile needs --consensus
    with pytest.raises(SystemExit):
        _cli.cli(["--ont", "--fastq", sq, "--outfolder", str(tmp_path / "x"), "--error_profile"])


def test_cli_flag_under_fastq_dir_and_with_recruit(gpu_api, tmp_path):
    import shutil
    d = tmp_path / "in"; d.mkdir()
    shutil.copy(os.path.join(GOLD, "sample_h1.fastq"), str(d / "h1.fastq"))
    synth.reads_to_fastq(synth.make_reads(synth.make_species(2, 600, 0.12, seed=81), 400, mu=15.0, seed=82, rc_fraction=0.3), str(d / "s_a.fastq"), prefix="a")
    _, plain = _run(gpu_api, tmp_path, "plain", ["--fastq_dir", str(d)], ["--recruit"])
    _, both = _run(gpu_api, tmp_path, "dir", ["--fastq_dir", str(d)], ["--recruit", "--error_profile"])
    new = sorted(set(both) - set(plain))
    assert new == sorted(["error_profile_all.tsv", "quality_calibration_all.tsv"] + [os.path.join(s, f) for s in ("h1", "s_a") for f in ("error_profile.tsv", "quality_calibration.tsv")])
    assert all(plain[f] == both[f] for f in plain if not f.endswith("logfile.txt"))
    cat = {"error_profile_all.tsv": [], "quality_calibration_all.tsv": []}
    for x, s in enumerate(("h1", "s_a")):
        _, alone = _run(gpu_api, tmp_path, "alone_" + s, ["--fastq", str(d / (s + ".fastq"))], ["--recruit", "--error_profile"])
        for f, allf in (("error_profile.tsv", "error_profile_all.tsv"), ("quality_calibration.tsv", "quality_calibration_all.tsv")):
            assert both[os.path.join(s, f)] == alone[f] and len(alone[f].decode().splitlines()) > 5
            for line in alone[f].decode().split("\n")[:-1]:
                head = line.split("\t")[0] in ("cluster_id", "q")
                if head and x: continue
                cat[allf].append("" if not line else ("sample" if head else s) + "\t" + line)
    for allf in cat:
        assert both[allf].decode().split("\n")[:-1] == cat[allf]
    # the lists are the recruited ones: every read assigned to a consensus is listed under it
    asg = [l.split("\t") for l in both[os.path.join("s_a", "read_assignments.tsv")].decode().splitlines()][1:]
    tab = errprof.read_table(str(tmp_path / "dir" / "s_a" / "error_profile.tsv"))
    for cid, t in tab["counts"].items():
        n_asg = sum(1 for x in asg if x[1] == cid and x[5] == "assigned")
        assert 0.9 * n_asg <= int(t[:, READS].sum()) <= n_asg and n_asg > 20
