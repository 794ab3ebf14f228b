"""CPU: tests/frontend_reference.py (plain Python, written from include/ngsid.h) against the reference program's own output in tests/golden/, and the
oracle against that reference on every case of tests/frontend_cases.py.  The GPU twin is test_gpu_frontend_reference.py."""
import math, os
from fractions import Fraction
import numpy as np
import pytest
from oracle_lib import GOLD
from ngspeciesid_amd._capi import ReadSet, NgsidError
import frontend_reference as fr
import frontend_cases as fc

SCORE_IDS = [c["name"] for c in fc.score_cases()]
MZ_IDS = [c["name"] for c in fc.minimizer_cases()]
EXACT = [i for i, c in enumerate(fc.score_cases()) if c["exact"]]          # (the two histogram sets hold reads beyond 4 000 bases: float replay only)
SCORE_NAMES, MZ_NAMES = ("score", "err", "keep"), ("mz_off", "codes", "pos", "hpc_len", "hpc_err")


def _load(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def _strings(buf, off):
    b = buf.tobytes().decode("latin-1")
    return [b[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def _ulp16(got, ref):
    return np.all(np.abs(got - ref) <= 16 * np.spacing(ref))


# ---------------------------------------------------------------------------------------------- the reference against the reference program's output
def test_reference_scores_equal_the_golden():
    g = _load("scores_sample_h1.npz")
    score, err, keep, _ = fr.scores_ref(_strings(g["seq"], g["off"]), _strings(g["qual"], g["off"]), int(g["k"]), 7.0)
    assert np.array_equal(keep, g["keep"])
    m = g["keep"] == 1
    assert m.sum() > 100
    assert np.array_equal(score[m], g["score"][m])
    assert _ulp16(err[m], g["err"][m])                      # the reference program sums in hash order


@pytest.mark.parametrize("tag", ["sample_h1", "synth200"])
def test_reference_minimizers_equal_the_golden(tag):
    g = _load("minimizers_%s.npz" % tag)
    seqs, quals = _strings(g["seq"], g["off"]), _strings(g["qual"], g["off"])
    assert [fr.hpc_string(s) for s in seqs] == _strings(g["hpc"], g["hpc_off"])
    for k, w in ((13, 20), (15, 50), (10, 100), (21, 21)):
        moff, codes, pos, hl, he = fr.call_ref(seqs, quals, k, w)
        assert np.array_equal(hl, np.diff(g["hpc_off"].astype(np.int64)))
        assert np.array_equal(moff, g["moff_%d_%d" % (k, w)]), (k, w)
        assert np.array_equal(codes, g["codes_%d_%d" % (k, w)]), (k, w)
        assert np.array_equal(pos, g["pos_%d_%d" % (k, w)]), (k, w)
        assert _ulp16(he, g["hpc_err"])


def test_reference_wide_k_ranks_equal_the_golden():
    g = _load("minimizers_widek.npz")
    seqs, quals = _strings(g["seq"], g["off"]), _strings(g["qual"], g["off"])
    for k, w in ((25, 30), (30, 35), (22, 22), (32, 40)):
        moff, codes, pos, hl, he = fr.call_ref(seqs, quals, k, w)
        assert np.array_equal(moff, g["moff_%d_%d" % (k, w)]), (k, w)
        assert np.array_equal(pos, g["pos_%d_%d" % (k, w)]), (k, w)
        assert np.array_equal(codes, g["rank_%d_%d" % (k, w)]), (k, w)


# ---------------------------------------------------------------------------------------------- by hand
def test_by_hand_empty_kmer_wins_a_window_longer_than_the_string(oracle):
    """k = 3, w = 8: W = 6 > k + 1.  h = ACG has the k-mers ACG, CG, G and three empty ones; the empty string sorts first, leftmost at 3 = len(h)"""
    assert fr.minimizers_ref("ACG", 3, 8) == [("", 3)]
    assert fr.codes_ref([""], 3) == [0]
    for got in (fr.call_ref(["AACGG"], ["IIIII"], 3, 8), oracle.hpc_minimizers(ReadSet.from_strings(["AACGG"], ["IIIII"]), 3, 8)):
        assert [a.tolist() for a in got[:4]] == [[0, 1], [0], [3], [3]]


def test_by_hand_equal_kmers_leftmost(oracle):
    """k = 2, w = 4 on ACACAC: k-mers AC CA AC CA AC, windows of three: {0,1,2} -> 0, {1,2,3} -> 2, {2,3,4} -> 2 (not 4).  AC = 1 * 8 + 2"""
    assert fr.minimizers_ref("ACACAC", 2, 4) == [("AC", 0), ("AC", 2)]
    for got in (fr.call_ref(["ACACAC"], None, 2, 4), oracle.hpc_minimizers(ReadSet.from_strings(["ACACAC"]), 2, 4)):
        assert [a.tolist() for a in got[:4]] == [[0, 2], [10, 10], [0, 2], [6]]
        assert math.isnan(got[4][0])
    # "AC" * n: the minimizer moves by two from window to window
    assert fr.minimizers_ref("AC" * 6, 2, 4) == [("AC", p) for p in (0, 2, 4, 6, 8)]


def test_by_hand_run_quality_tie(oracle):
    """AAA with the qualities ' ', '!', '!' (one P for all three): the run's quality is the first, ' '.  CC with '5', 'I': 'I' has the lower P.
    HPC error rate = (P[' '] + P['I']) / 2 = (0.79433 + 0.0001) / 2"""
    h, hq, e = fr.hpc_ref("AAACC", " !!5I")
    assert (h, hq) == ("AC", " I")
    assert e == 0.397215
    assert oracle.hpc_minimizers(ReadSet.from_strings(["AAACC"], [" !!5I"]), 1, 1)[4][0] == 0.397215
    assert fr.hpc_ref("AAACC", "I5I5I")[1] == "II"


def test_by_hand_scores():
    """k = 1 and every quality '+' (Q10, P = 0.1): every window holds 0.9, the score is 0.9 per base; '!' is clamped to 0.79433 in the product and
    not in the error rate, which is exactly 1 (phred -0.0: dropped at any threshold >= 0)"""
    assert fr.P[43] == 0.1 and fr.RAW[43] == 0.1 and fr.P[33] == 0.79433 and fr.RAW[33] == 1.0
    s, e, keep = fr.score_ref("ACGT", "++++", 1, 7.0)
    assert abs(s - 3.6) <= 4 * math.ulp(4.0) and e == 0.1 and keep == 1
    s, e, keep = fr.score_ref("ACGT", "!!!!", 2, 7.0)
    assert abs(s - 3 * (1 - 0.79433) ** 2) < 1e-15 and e == 1.0 and keep == 0
    assert fr.score_ref("ACG", "+++", 2, 7.0) == (0.0, 0.0, 0)               # shorter than 2k
    assert fr.score_ref("AAAAAAC", "+++++++", 3, 7.0)[2] == 0 and fr.score_ref("AAAAACG", "+++++++", 3, 7.0)[2] == 1      # HPC length 2 < k, 3 = k
    assert fr.score_exact("++++", 2) == 3 * (1 - Fraction(0.1)) ** 2


# ---------------------------------------------------------------------------------------------- the oracle against the reference
@pytest.mark.parametrize("i", range(len(SCORE_IDS)), ids=SCORE_IDS)
def test_oracle_scores_equal_the_reference(oracle, i):
    """score and err bit for bit; keep for every read but the one built to sit ON the threshold (there the last bit of log() decides)"""
    c = fc.score_cases()[i]
    score, err, keep, phred = fc.score_expected(i)
    got = oracle.score_reads(fc.read_set(c), c["k"], c["thr"])
    on = np.array([t == "on" for t in c["tags"]])
    msg = fc.first_difference(c, (got[0], got[1], got[2][~on]), (score, err, keep[~on]), SCORE_NAMES, per_read=SCORE_NAMES[:2])
    assert msg is None, msg


def test_keep_is_compared_everywhere_but_on_the_threshold():
    """the reads the reference places within 1e-9 of the threshold are exactly the six built to be there (one per k); their neighbours are decided"""
    near, on = [], []
    for i, c in enumerate(fc.score_cases()):
        score, err, keep, phred = fc.score_expected(i)
        for r, t in enumerate(c["tags"]):
            if abs(phred[r] - c["thr"]) <= 1e-9: near.append((c["name"], r))
            if t == "on": on.append((c["name"], r))
            if t == "above": assert keep[r] == 1 and 1e-4 < phred[r] - c["thr"] < 1e-2
            if t == "below": assert keep[r] == 0 and 1e-4 < c["thr"] - phred[r] < 1e-2
    assert near == on and len(on) == len(fc.SCORE_KS) == 6


@pytest.mark.parametrize("i", EXACT, ids=[SCORE_IDS[i] for i in EXACT])
def test_float_replay_stays_within_the_derived_bound_of_the_exact_sum(oracle, i):
    """|score - exact| <= 5 L 2^-53 N + 4 ulp(N), L = read length, N = L - k + 1, exact = the sum over the N windows of the exact product of (1 - P[q]).

    Derivation, u = 2^-53 (round to nearest).  A step of the recurrence rounds four times - 1 - p_new, 1 - p_old, their quotient, its product with cur
    (the first k steps twice) - so after i steps cur carries a relative error of at most (1 + u)^(4i) - 1 <= 4 L u (1 + 1e-11); every window product
    lies in (0, 1], so the N terms are wrong by at most 4 L u each, 4 L u N together.  The running sum adds one rounding per term; all terms are
    positive, so the sum of at most N <= L terms is wrong by at most L u times its value <= N: together 5 L u N.  score = (1 - (N - sum) / N) * N rounds
    four more times, each result being at most N, or at most 1 and then multiplied by N: half an ulp of N each.  The second-order terms are
    below 1e-11 of the first.  A kernel or oracle that loses the recurrence (wrong leaving character, restart at a slice) misses by many orders of magnitude.
    Measured with the reference's own floats: the worst read uses 6.2 % of the bound (printed per case)."""
    c = fc.score_cases()[i]
    k = c["k"]
    score = fc.score_expected(i)[0]
    oscore = oracle.score_reads(fc.read_set(c), k, c["thr"])[0]
    worst = 0.0
    for r, (s, q) in enumerate(zip(c["seqs"], c["quals"])):
        L = len(s); N = L - k + 1
        if L < 2 * k or len(fr.hpc_string(s)) < k: continue
        assert L <= 4000
        exact = fr.score_exact(q, k)
        bound = 5 * L * 2.0 ** -53 * N + 4 * math.ulp(float(N))
        for what, v in (("reference", score[r]), ("oracle", oscore[r])):
            d = abs(Fraction(float(v)) - exact)
            worst = max(worst, float(d) / bound)
            assert d <= Fraction(bound), "%s: %s score of %s is %r, exact %r, bound %.3g" % (c["name"], what, fc.describe_read(c, r), float(v), float(exact), bound)
    print("%s: worst |score - exact| / bound = %.4f" % (c["name"], worst))


@pytest.mark.parametrize("i", range(len(MZ_IDS)), ids=MZ_IDS)
def test_oracle_minimizers_equal_the_reference(oracle, i):
    c = fc.minimizer_cases()[i]
    exp = fc.minimizer_expected(i)
    if c["bad"]:
        assert isinstance(exp, fr.AlphabetError) and exp.reads == c["bad"]
        with pytest.raises(NgsidError) as e:
            oracle.hpc_minimizers(fc.read_set(c), c["k"], c["w"])
        assert e.value.code == -3 and ("read %d:" % c["bad"][0]) in str(e.value)          # sequential: the first one
        return
    got = oracle.hpc_minimizers(fc.read_set(c), c["k"], c["w"])
    msg = fc.first_difference(c, got, exp, MZ_NAMES, per_read=MZ_NAMES[3:])
    assert msg is None, msg


def test_cases_cover_what_they_are_for():
    """the properties the shapes were chosen for do occur: truncated and empty k-mers among the minimizers, every window count, both code widths"""
    trunc = empty = 0
    Ws = set()
    for i, c in enumerate(fc.minimizer_cases()):
        if c["bad"] or not c["name"].endswith("main"): continue
        k, w = c["k"], c["w"]; Ws.add(w - k + 1)
        moff, codes, pos, hl, he = fc.minimizer_expected(i)
        for r in range(len(hl)):
            for p in pos[int(moff[r]):int(moff[r + 1])]:
                trunc += int(p) + k > int(hl[r]); empty += int(p) == int(hl[r])
        assert (hl == 0).any() and (hl == 1).any() and np.isnan(he).sum() == (hl == 0).sum()
        if k > 21:
            assert len(np.unique(codes)) < len(codes) and int(codes.max()) == len(np.unique(codes)) - 1            # dense, with repeats
    assert Ws >= {1, 2, 16, 17, 32, 33, 64, 65, 255} and trunc > 50 and empty > 5
    assert fc.tie_read()[1].count(" ") >= 1
    # score cases: every start x length residue mod 4 occurs in the offset sets
    for c in fc.score_cases():
        if c["name"].endswith("offsets"):
            at, seen = 0, set()
            for s in c["seqs"]:
                if len(s) > 3: seen.add((at % 4, len(s) % 4))
                at += len(s)
            assert len(seen) == 16


def test_score_k_above_64_is_an_argument_error_of_the_library_only():
    """ngsid_score_reads refuses k = 65 (NGSID_ERR_ARG, tested on the GPU); the reference has no such limit: its ring is the string"""
    s, e, keep = fr.score_ref("ACGT" * 40, "5" * 160, 65, 7.0)
    assert keep == 1 and 0 < s < 96
