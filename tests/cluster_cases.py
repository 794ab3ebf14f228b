"""Deterministic adversarial read sets for the greedy clustering stage (csrc/k_cluster.hip, oracle/ngsid_oracle.c: ongsid_cluster_greedy).

Every case is built to reach ONE named mechanism of the block driver that natural reads almost never reach.  Pure numpy / Python, seeded; the only helper is the CPU oracle's
minimizer routine (oracle.hpc_minimizers), used to MEASURE shared minimizers while a case is constructed (rejection sampling until a count is hit).  The sequences are frozen in
tests/golden/cluster_edges.npz (oracle/make_golden_cluster_edges.py) together with the verdict of the reference's own reads_to_clusters; tests/test_cluster_edges_cpu.py checks
that these generators still reproduce the frozen reads byte for byte.

All sequences have no two equal neighbouring letters, so homopolymer compression is the identity and a read's HPC length is its length.

A Case holds the reads and a list of calls.  One call = one invocation of cluster_greedy: cluster parameters, optional prev_batch / known_err, and the p-table
("select": ptable.select_p_table(k, w); "round2": round2_table(known_err[1], known_err[0]), see case (a))."""
import math
import numpy as np
from ngspeciesid_amd._capi import ReadSet
from ngspeciesid_amd.ptable import select_p_table

PRM_DEFAULT = dict(min_shared=5, symmetric=0, min_fraction=0.8, mapped_threshold=0.7, aligned_threshold=0.4, min_prob_no_hits=0.1)
PRM_KEYS = ("min_shared", "symmetric", "min_fraction", "mapped_threshold", "aligned_threshold", "min_prob_no_hits")
Q40, Q10 = "I", "+"           # phred 40 (p = 1e-4, table row 1) and phred 10 (p = 0.1, table row 10)


class Call:
    def __init__(self, tag, prm=None, prev_batch=None, known_err=None, ptab="select"):
        self.tag = tag; self.prm = dict(PRM_DEFAULT, **(prm or {})); self.ptab = ptab
        self.prev_batch = None if prev_batch is None else np.asarray(prev_batch, dtype=np.int32)
        self.known_err = None if known_err is None else np.asarray(known_err, dtype=np.float64)


class Case:
    def __init__(self, name, seqs, quals=None, k=13, w=20, calls=None, acc=None, info=None):
        self.name, self.seqs, self.k, self.w = name, list(seqs), k, w
        self.quals = list(quals) if quals is not None else [Q40 * len(s) for s in self.seqs]
        self.acc = list(acc) if acc is not None else ["r%04d" % i for i in range(len(self.seqs))]
        self.calls = calls or [Call("default")]
        self.info = info or {}          # positions / read numbers the conditions of test_cluster_edges_cpu.py look at


# ------------------------------------------------------------------------------------------------ sequence helpers
def rnd_seq(rng, L):
    steps = rng.integers(1, 4, L); steps[0] = rng.integers(0, 4)
    return "".join("ACGT"[x] for x in np.cumsum(steps) % 4)


def substitute(rng, s, positions):
    """substitutions at `positions` that keep neighbouring letters different (HPC stays the identity)"""
    a = list(s)
    for p in positions:
        ban = {a[p]} | ({a[p - 1]} if p else set()) | ({a[p + 1]} if p + 1 < len(a) else set())
        ch = [c for c in "ACGT" if c not in ban]
        a[p] = ch[int(rng.integers(0, len(ch)))]
    return "".join(a)


def join(*parts):
    """concatenation without a homopolymer at a seam: the first letter of a part is changed if it repeats the letter before it (and stays different from its successor)"""
    out = ""
    for p in parts:
        if out and p and p[0] == out[-1]:
            ban = {out[-1]} | ({p[1]} if len(p) > 1 else set())
            p = [c for c in "ACGT" if c not in ban][0] + p[1:]
        out += p
    return out


def minimizers(oracle, seqs, k=13, w=20):
    """[(codes, pos)] per read"""
    moff, codes, pos, hl, _ = oracle.hpc_minimizers(ReadSet.from_strings(list(seqs), [Q40 * len(s) for s in seqs]), k, w)
    assert all(int(h) == len(s) for h, s in zip(hl, seqs)), "a generated sequence holds a homopolymer"
    return [(codes[int(moff[i]):int(moff[i + 1])], pos[int(moff[i]):int(moff[i + 1])]) for i in range(len(seqs))]


def hits(read_mz, rep_mz):
    """(number, sum of positions, indices) of the read's minimizers found in the representative: the candidate key of cluster.py:79"""
    inset = np.isin(read_mz[0], np.unique(rep_mz[0]))
    return int(inset.sum()), int(read_mz[1][inset].astype(np.int64).sum()), np.nonzero(inset)[0]


def mapped_ratio(read_mz, rep_mz, hlen, p_shared, min_prob=0.1):
    """get_best_cluster's mapped span (cluster.py:97-117), used only to steer the construction of case (e)"""
    n, _, idx = hits(read_mz, rep_mz)
    if n == 0: return 0.0
    perr, M, pos, tot = 1.0 - p_shared, len(read_mz[0]), read_mz[1].astype(np.int64), 0
    ok = lambda gap: perr ** gap >= min_prob
    for t in range(n + 1):
        gap = idx[0] if t == 0 else (M - 1 - idx[-1] if t == n else idx[t] - idx[t - 1] - 1)
        if not ok(int(gap)): continue
        tot += pos[idx[0]] if t == 0 else (hlen - pos[idx[-1]] if t == n else pos[idx[t]] - pos[idx[t - 1]])
    return tot / float(hlen)


# ------------------------------------------------------------------------------------------------ (a) round2_boundaries
def round2_index(e):
    """p_shared_minimizer_empirical's row / column, by CPython's own round() and the clamp (cluster.py:356-366); 1 .. 15"""
    r = round(float(e), 2)          # a Python float: numpy.float64.__round__ is another algorithm
    if r > 0.15: r = 0.15
    if r < 0.01: r = 0.01
    return int(round(r * 100))


def round2_table(e_read, e_rep):
    """A deliberately asymmetric table for ONE (read, representative) pair: p = 0 in the cell the reference reads (every gap tolerated: the pair maps), p = 1 in the
    cells one row / one column away (no gap tolerated: the pair of case (a) does not map), NaN everywhere else - the transposed cell included (NGSID_ERR_NO_PTABLE, the
    reference's KeyError).  So the read's status, or the error, tells which cell an implementation read."""
    i, j = round2_index(e_read), round2_index(e_rep)
    t = np.full((15, 15), np.nan)
    for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        if 1 <= i + di <= 15 and 1 <= j + dj <= 15: t[i + di - 1, j + dj - 1] = 1.0
    t[i - 1, j - 1] = 0.0
    return t.reshape(225)


def flip_point(nominal):
    """the smallest double that round(., 2) takes UP at the boundary `nominal` = x.xx5"""
    up = round(nominal + 0.004, 2)
    d = nominal
    while round(d, 2) < up: d = math.nextafter(d, 1.0)
    while round(math.nextafter(d, 0.0), 2) >= up: d = math.nextafter(d, 0.0)
    return d


def round2_points():
    """error rates at every boundary of round(e, 2) that the 15 x 15 table can see: 0.005 (both sides clamp to row 1), 0.015 ... 0.145 (the 14 row changes), 0.155 (both sides
    clamp to row 15) - the largest double below the flip, the flip, the next double above - and the far ends of both clamps"""
    pts = []
    for b in range(16):
        f = flip_point((2 * b + 1) / 200.0)
        pts += [math.nextafter(f, 0.0), f, math.nextafter(f, 1.0)]
    return pts + [0.0, 0.79433, 1.0]


def case_round2(oracle):
    rng = np.random.default_rng(101)
    rep = rnd_seq(rng, 300)
    read = join(rep[:100], rnd_seq(rng, 100), rep[200:])          # differs in a middle stretch: gaps exist, so p = 0 and p = 1 give different statuses
    calls = []
    for axis in ("read", "rep"):
        for n, e in enumerate(round2_points()):
            other = 0.12 if round2_index(e) < 8 else 0.03           # far from the varied index: the transposed cell is another cell
            er, ec = (e, other) if axis == "read" else (other, e)
            calls.append(Call("%s%02d" % (axis, n), prev_batch=[1, 2], known_err=[ec, er], ptab="round2"))
    return [Case("round2_boundaries", [rep, read], calls=calls)]


# ------------------------------------------------------------------------------------------------ (b) tied_candidates_beyond_cache
def case_tied(oracle):
    """six representatives end in the same 90-base core (unrelated 200-base heads); the query starts with the core.  Every minimizer the query shares with one of them lies in a
    window that is the same in all six, so (hits, sum of positions) is tied six ways; the core is too short for the mapping (90 / 290) and the alignment criterion.  One more
    founder in FRONT of the query shares a stretch of the query's tail: it is tentative when the query is decided first (six pairs, the 4-entry cache wraps), then committed, and
    the query is decided again."""
    for seed in range(200, 260):
        rng = np.random.default_rng(seed)
        core = rnd_seq(rng, 90)
        reps = [join(rnd_seq(rng, 200), core) for _ in range(6)]
        tail = rnd_seq(rng, 200)
        query = join(core, tail)
        mz = minimizers(oracle, reps + [query])
        keys = {hits(mz[6], mz[i])[:2] for i in range(6)}
        if len(keys) != 1: continue
        top = keys.pop()[0]
        for L in range(40, 160):
            late = join(rnd_seq(np.random.default_rng(seed * 1000 + L), 200), tail[200 - L:])
            n = hits(mz[6], minimizers(oracle, [late])[0])[0]
            if n == top:
                return [Case("tied_candidates_beyond_cache", reps + [late, query], info=dict(query=7, top=top))]
    raise AssertionError("no tie found")


# ------------------------------------------------------------------------------------------------ (c) accession_tiebreak
def case_accession(oracle):
    """two representatives end in the same 120-base core; a query that IS the core maps to either with the same (hits, sum of positions), a query core + own tail fails the
    mapping and passes the alignment against either.  The accessions are ordered against the slots: the reference's reversed sort takes the LATER representative."""
    rng = np.random.default_rng(301)
    core = rnd_seq(rng, 120)
    r1, r2 = join(rnd_seq(rng, 200), core), join(rnd_seq(rng, 200), core)
    qmap, qaln = core, join(core, rnd_seq(rng, 100))
    mz = minimizers(oracle, [r1, r2, qmap, qaln])
    for q in (2, 3): assert hits(mz[q], mz[0])[:2] == hits(mz[q], mz[1])[:2] and hits(mz[q], mz[0])[0] >= 5
    return [Case("accession_tiebreak", [r1, r2, qmap, qaln], acc=["a_first", "b_second", "c_qmap", "d_qaln"], info=dict(qmap=2, qaln=3, low=0, high=1))]


# ------------------------------------------------------------------------------------------------ (d) threshold_equalities
def case_thresholds(oracle):
    """a representative of 300 bases, a shorter read that maps (ratio r) and a shorter read that fails the mapping and passes the alignment (ratio a); both shorter than the
    representative, so with symmetric thresholds the representative-side ratio is the smaller one.  The calls at r / a and one double beside them are derived from the
    reference's trace by oracle/make_golden_cluster_edges.py and live in the fixture (THRESHOLD_CALLS names them)."""
    rng = np.random.default_rng(401)
    rep = rnd_seq(rng, 300)
    qm = substitute(rng, rep[10:290], [60, 150, 230])
    qa = join(rep[:150], rnd_seq(rng, 90))
    return [Case("threshold_equalities", [rep, qm, qa], calls=[Call("base"), Call("base_sym", prm=dict(symmetric=1))], info=dict(qm=1, qa=2))]


THRESHOLD_CALLS = ("map_at_r", "map_below_r", "aln_at_a", "aln_above_a", "sym_map_at_r", "sym_map_below_r", "sym_aln_at_a", "sym_aln_above_a")


def threshold_calls(r, a, r_sym, a_sym):
    """the derived calls of case (d): strict > at the mapping ratio, >= at the alignment ratio"""
    s = dict(symmetric=1)
    return [Call("map_at_r", prm=dict(mapped_threshold=r)), Call("map_below_r", prm=dict(mapped_threshold=math.nextafter(r, 0.0))),
            Call("aln_at_a", prm=dict(aligned_threshold=a)), Call("aln_above_a", prm=dict(aligned_threshold=math.nextafter(a, 1.0))),
            Call("sym_map_at_r", prm=dict(s, mapped_threshold=r_sym)), Call("sym_map_below_r", prm=dict(s, mapped_threshold=math.nextafter(r_sym, 0.0))),
            Call("sym_aln_at_a", prm=dict(s, aligned_threshold=a_sym)), Call("sym_aln_above_a", prm=dict(s, aligned_threshold=math.nextafter(a_sym, 1.0)))]


# ------------------------------------------------------------------------------------------------ (e) fraction_boundary
def case_fraction(oracle):
    """reads A, B, X at phred 10 (table row 10: p = 0.165, runs of up to 12 missed minimizers are bridged).  X starts with 55 bases of A (t shared minimizers, too few bases
    for either criterion) and goes on with 245 bases of which B holds a copy with spaced substitutions: few shared minimizers, spread over the whole stretch, so X maps to B
    (mapped_threshold = 0.5: a handful of spread hits bridges somewhat more than half of X) and aligns to B.  B is founded in the same block, in front of X, after X was decided against A.  The substitutions are drawn until X and B share exactly
    ceil(f t) - 1 (B cannot matter), ceil(f t) (B is visited) or t + 1 minimizers (B is the new top), f = min(min_fraction, 1).  In the "visited" case of f = 0.8, t is a
    multiple of 5, so that B sits exactly AT f t."""
    p10 = float(select_p_table(13, 20)[9 * 15 + 9])
    out = []
    for mf in (0.8, 1.2):
        for which in ("below", "at", "top"):
            found = None
            for seed in range(500, 4000):
                rng = np.random.default_rng(seed)
                a = rnd_seq(rng, 300); z = rnd_seq(rng, 245); head = rnd_seq(rng, 100)
                x = join(a[:55], z)
                mz = minimizers(oracle, [a, x])
                t = hits(mz[1], mz[0])[0]
                if t < 8 or (which == "at" and mf == 0.8 and t % 5): continue      # f t is a whole number there: the reference's strict < (cluster.py:88) keeps B, <= would not
                c = int(math.ceil(min(mf, 1.0) * t))
                target = {"below": c - 1, "at": c, "top": t + 1}[which]
                nsub = int(rng.integers(20, 46))
                b = join(head, substitute(rng, z, sorted(rng.choice(np.arange(2, 243), nsub, replace=False).tolist())))
                mb = minimizers(oracle, [b])[0]
                if hits(mz[1], mb)[0] != target or hits(mb, mz[0])[0] != 0: continue
                if mapped_ratio(mz[1], mb, len(x), p10) <= 0.55 or mapped_ratio(mz[1], mz[0], len(x), p10) >= 0.3: continue      # (clear of mapped_threshold = 0.5 on both sides)
                found = Case("fraction_boundary_%s_mf%02d" % (which, int(mf * 10)), [a, b, x], quals=[Q10 * len(s) for s in (a, b, x)],
                             calls=[Call("default", prm=dict(min_fraction=mf, mapped_threshold=0.5))], info=dict(x=2, a=0, b=1, t=t, target=target, which=which, mf=mf))
                break
            assert found is not None, (mf, which)
            out.append(found)
    return out


# ------------------------------------------------------------------------------------------------ (f) dependent_chain
def case_chain(oracle):
    """200 reads; read i = Y[i-1] + U[i] + Y[i] (60 bases each): it shares its first third with its predecessor only - enough minimizers to be looked at, a third of the read is
    too little for either criterion - so every read founds a cluster and every restart round can commit a single representative"""
    rng = np.random.default_rng(601)
    n = 200
    y = [rnd_seq(rng, 60) for _ in range(n + 1)]
    seqs = [join(y[i], rnd_seq(rng, 60), y[i + 1]) for i in range(n)]
    mz = minimizers(oracle, seqs)
    for i in range(1, n):
        tries = 0
        while hits(mz[i], mz[i - 1])[0] < 5:          # (a seam moved a minimizer: draw the shared third again)
            tries += 1; assert tries < 50
            y[i] = rnd_seq(rng, 60)
            seqs[i - 1] = join(y[i - 1], seqs[i - 1][60:120], y[i]); seqs[i] = join(y[i], seqs[i][60:120], y[i + 1])
            mz = minimizers(oracle, seqs)
    return [Case("dependent_chain", seqs)]


# ------------------------------------------------------------------------------------------------ (g) many_founders
def case_founders(oracle):
    """600 unrelated founders (80 - 120 bases) with 26 joiners strewn over items 300 - 511, then 60 joiners: more than 64 new representatives in one pass, and with
    cluster_block = 512 more than 256 new representatives inside one block (the hit matrix regrows with lo > b0, and reads behind the regrowth still join early founders)"""
    rng = np.random.default_rng(701)
    founders = [rnd_seq(rng, int(rng.integers(80, 121))) for _ in range(600)]

    def joiner(upto):
        f = founders[int(rng.integers(0, upto))]
        return f if rng.random() < 0.5 else substitute(rng, f, [len(f) // 2])
    seqs, nf = [], 0
    while nf < 600:
        if nf >= 300 and len(seqs) < 512 and len(seqs) % 8 == 7: seqs.append(joiner(nf)); continue
        seqs.append(founders[nf]); nf += 1
    seqs += [joiner(600) for _ in range(60)]
    return [Case("many_founders", seqs)]


# ------------------------------------------------------------------------------------------------ (h) word_boundaries
WORD_COUNTS = (63, 64, 65, 127, 128, 129, 191)


def case_words(oracle):
    """item counts around the 64-item mask words.  New representatives at items 0, 63, 64, 127 and the last one; item 64 shares the last 70 bases of item 63 (affected by
    it while it is tentative, founds its own cluster), item 65 is a copy of item 64 (joins a representative that was tentative one round earlier).  The same pair of items at
    20 / 21 and 100 / 101 restarts the block in the middle of a word (lo - b0 not a multiple of 64, for block sizes 64 and 128 alike).  Everything else is a copy of item 0
    with two substitutions."""
    out = []
    for n in WORD_COUNTS:
        rng = np.random.default_rng(800 + n)
        f0 = rnd_seq(rng, 150)
        seqs = [substitute(rng, f0, sorted(rng.choice(np.arange(5, 145), 2, replace=False).tolist())) for _ in range(n)]
        seqs[0] = f0
        founders = [0]
        for p in (20, 63, 100, 127):
            if p < n: seqs[p] = rnd_seq(rng, 150); founders.append(p)
            if p + 1 < n and p != 127: seqs[p + 1] = join(seqs[p][-70:], rnd_seq(rng, 130)); founders.append(p + 1)
            if p + 2 < n and p != 127: seqs[p + 2] = substitute(rng, seqs[p + 1], [100])
        if n - 1 not in founders: seqs[n - 1] = rnd_seq(rng, 150); founders.append(n - 1)
        out.append(Case("word_boundaries_n%d" % n, seqs, info=dict(founders=sorted(founders))))
    return out


# ------------------------------------------------------------------------------------------------ (i) dense_long_founder
DENSE_LENGTHS = (25000, 16397, 16396)      # k = w = 13: every k-mer is a minimizer; 16 396 bases = 16 384 minimizers, the last size the in-LDS sort of a representative holds


def case_dense(oracle):
    """one long founder at k = w = 13, two copies with 1 % and 2 % substitutions and two excerpts that must join it, three short unrelated reads that must not"""
    out = []
    for L in DENSE_LENGTHS:
        rng = np.random.default_rng(900 + L)
        f = rnd_seq(rng, L)
        c1 = substitute(rng, f, sorted(rng.choice(np.arange(1, L - 1), L // 100, replace=False).tolist()))
        c2 = substitute(rng, f, sorted(rng.choice(np.arange(1, L - 1), L // 50, replace=False).tolist()))
        seqs = [f, rnd_seq(rng, 200), c1, f[L // 2:L // 2 + 300], rnd_seq(rng, 100), c2, f[-200:], rnd_seq(rng, 300)]
        out.append(Case("dense_long_founder_%d" % L, seqs, k=13, w=13, info=dict(join=[2, 3, 5, 6], alone=[1, 4, 7])))
    return out


# ------------------------------------------------------------------------------------------------ (j) merge_round_edges
def case_merge(oracle):
    """merge-round inputs (cluster.py:221-223, 243-248, 273-277).  Reads 0 - 2 are lower-batch representatives (read 2: HPC length k - 1, never indexed), 3 - 4 carry batch 0
    in one call, the rest are higher-batch representatives: a copy of read 0 (re-clustered into it), a copy of read 1 with a substitution every 40 bases (maps only when the
    KNOWN error rate 0.12 puts both in table row 12, not with the error rate its qualities give), an unrelated read and its copy, and reads of HPC length k - 1, k and k + 1."""
    rng = np.random.default_rng(1001)
    s0, s1, u = rnd_seq(rng, 300), rnd_seq(rng, 320), rnd_seq(rng, 250)
    seqs = [s0, s1, rnd_seq(rng, 12), rnd_seq(rng, 200), substitute(rng, s0, [150]), substitute(rng, s0, [40, 200]), substitute(rng, s1, list(range(20, 320, 40))),
            u, substitute(rng, u, [100]), rnd_seq(rng, 12), rnd_seq(rng, 13), rnd_seq(rng, 14)]
    n = len(seqs)
    _, _, _, _, he = oracle.hpc_minimizers(ReadSet.from_strings(seqs, [Q40 * len(s) for s in seqs]), 13, 20)
    nan = np.full(n, np.nan)
    seeded = np.array([1, 1, 1] + [2] * (n - 3))
    differs = he.copy(); differs[1] = differs[6] = 0.12
    only_seeds = nan.copy(); only_seeds[:3] = he[:3]
    calls = [Call("all_seeded", prev_batch=np.ones(n), known_err=he),
             Call("mixed", prev_batch=seeded, known_err=he),
             Call("items_unknown", prev_batch=seeded, known_err=only_seeds),
             Call("zeros", prev_batch=np.array([1, 1, 1, 0, 0] + [2] * (n - 5)), known_err=he),
             Call("lowest_two", prev_batch=seeded + 1, known_err=he),
             Call("known_differs", prev_batch=seeded, known_err=differs)]
    return [Case("merge_round_edges", seqs, calls=calls, info=dict(sparse=6))]


# ------------------------------------------------------------------------------------------------ degenerate hit lists
def case_single_hit(oracle):
    """min_shared = 1: a read whose ONLY hit is its first minimizer (it starts with the first 20 bases of the representative) and one whose only hit is its last
    (it ends with the last 20): hit lists of length one at index 0 and at index M - 1, where the leading / trailing gap of get_best_cluster (cluster.py:101) is empty"""
    for seed in range(1100, 1400):
        rng = np.random.default_rng(seed)
        rep = rnd_seq(rng, 200)
        first, last = join(rep[:20], rnd_seq(rng, 180)), join(rnd_seq(rng, 180), rep[-20:])
        mz = minimizers(oracle, [rep, first, last])
        if hits(mz[1], mz[0])[2].tolist() == [0] and hits(mz[2], mz[0])[2].tolist() == [len(mz[2][0]) - 1] and hits(mz[2], mz[1])[0] == 0:
            return [Case("single_hit_ends", [rep, first, last], calls=[Call("min_shared_1", prm=dict(min_shared=1))])]
    raise AssertionError("no such reads")


def all_cases(oracle):
    out = []
    for f in (case_round2, case_tied, case_accession, case_thresholds, case_fraction, case_chain, case_founders, case_words, case_dense, case_merge, case_single_hit):
        out += f(oracle)
    return out


# ------------------------------------------------------------------------------------------------ the frozen form (tests/golden/cluster_edges.npz)
class Frozen:
    """one case as the fixture holds it: the reads, and per call the inputs and the reference's verdict.  The GPU tests read nothing else."""
    def __init__(self, g, name):
        p = name + "__"
        self.name = name
        self.rs = ReadSet(g[p + "seq"], g[p + "qual"], g[p + "off"])
        self.acc = [str(a) for a in g[p + "acc"]]
        self.k, self.w = (int(x) for x in g[p + "kw"])
        self.tags = [str(t) for t in g[p + "tags"]]
        self.f = {key: g[p + key] for key in ("prm", "ptab_round2", "has_prev", "has_known", "prev", "known", "rep_of", "status", "tr_best", "tr_ns", "tr_ratio", "counters", "pairs", "error")}
        order = np.argsort(np.array(self.acc, dtype=object), kind="stable")
        self.acc_rank = np.zeros(len(self.acc), dtype=np.uint32); self.acc_rank[order] = np.arange(len(self.acc), dtype=np.uint32)      # accessions are distinct

    def call(self, c):
        """(cluster_params, keyword arguments) of call c"""
        from ngspeciesid_amd._capi import cluster_params
        v = dict(zip(PRM_KEYS, self.f["prm"][c]))
        known = self.f["known"][c] if self.f["has_known"][c] else None
        tab = round2_table(known[1], known[0]) if self.f["ptab_round2"][c] else select_p_table(self.k, self.w)
        prm = cluster_params(k=self.k, w=self.w, min_shared=int(v["min_shared"]), min_fraction=v["min_fraction"], mapped_threshold=v["mapped_threshold"],
                             aligned_threshold=v["aligned_threshold"], min_prob_no_hits=v["min_prob_no_hits"], symmetric=bool(v["symmetric"]), p_shared=tab)
        return prm, dict(acc_rank=self.acc_rank, prev_batch=self.f["prev"][c] if self.f["has_prev"][c] else None, known_err=known)


def load_frozen():
    import os
    from oracle_lib import GOLD
    g = np.load(os.path.join(GOLD, "cluster_edges.npz"), allow_pickle=False)
    return [Frozen(g, str(n)) for n in g["cases"]]
