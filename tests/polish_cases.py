"""Deterministic polishing groups (fixed seeds) for the whole-call anchor: tests/test_polish_reference_cpu.py and tests/test_gpu_polish_reference.py.

A group = one backbone, 0 - 8 reads, optionally qualities, and the parameters of its call.  As in poa_cases.py the reads and the backbone differ from one template
only at VARIANT SITES (template without equal neighbours, sites at least 7 bases apart, at least 7 bases from the ends of any read and at least GUARD bases from every
window edge), so that a window's consensus is a set of real votes and the reference rarely has to break a tie (polish_reference reports when it did).  A site is
either PLANTED - the backbone carries the error, every read the template - or a VOTE, where backbone and reads draw their allele.  With a site every ~14 bases and
vote probabilities of 0.15 - 0.85 a read differs from its template by 2 - 4 %.

Families (W = 200 unless stated; all paths stay within a few columns of the diagonal and groups have at most 8 reads: far inside the default band and node capacity,
which have tests of their own):
  a_geometry   backbone lengths around every window rule (tail of 19 merges, tail of 20 does not), full-length reads
  b_edges      Bl = 600: reads that start / end at window edges +-{0..3} (both sides of the 1 % slack rule), reach 3 and 4 bases into a window (0.02 W = 4: dropped / kept),
               overhang the backbone's ends by 1 - 30 bases; windows 1 and 2 begin with a doubled base (a four-base layer needs a place of its own); in every sixth
               group the backbone's last base of window 0 is wrong and every layer there is end-free; every group twice: aln_mode 2 / trim 2 and aln_mode 3 / trim 3
  c_filters    layers whose quality sum is 10 len, 10 len - 1, 10 len + 1; the same as FASTA; quality '!'; reads with one long deletion so that (read span, backbone span)
               = (140, 200), (70, 100), (139, 200), (141, 200): the deleted stretch is a run of A inside a template of C / G / T, so that no read base can match
               there and the long deletion is the one optimal alignment
  d_strands    half the reads reverse-complemented, reads with N, unrelated reads, groups of unrelated reads only, of 0 and of 1 read, backbones shorter than k, k above 21,
               w below k, a read that is half forward and half reverse complement
  e_trim       W = 500, three reads of mean length exactly 1000 / 1001 that stop 5 - 40 bases short of the backbone's ends, each group under trim 0 1 2 3
  f_iterations iters = 3, backbones of 418 - 422 bases with planted indels that the reads undo: the tail crosses the W / 10 boundary between iterations
The seed of a group is its index unless SEEDS names another one: seeds were chosen so that polish_reference ALONE calls enough groups decided (the CPU test asserts the
share); no other implementation's output took part in the choice.
"""
import numpy as np
import ed_reference as ed
import poa_cases as pc
import polish_reference as ref

GUARD = 12
KINDS = ("del", "ins", "sub")
BASE = dict(iters=2, window=200, quality_threshold=10.0, error_threshold=0.3, match=3, mismatch=-5, gap=-4, k=13, w=20, trim=2, aln_mode=2)
A_LENGTHS = (150, 199, 200, 201, 219, 220, 221, 400, 401, 419, 420, 421, 619)
SEEDS = {("b_edges", 3): 303, ("b_edges", 4): 204, ("b_edges", 6): 406, ("b_edges", 7): 107, ("b_edges", 11): 111}


class Group:
    def __init__(self, name, backbone, reads, quals, prm, template=None):
        self.name, self.backbone, self.reads, self.quals, self.prm, self.template = name, backbone, reads, quals, dict(prm), template


def _rng(fid, gi, seed):
    return np.random.default_rng([20250311, fid, gi, seed])


def _sites(rng, t, W, lo=0, hi=None, step=12):
    """variant sites of template t (a list; del / ins / sub leave it as it is) -> [(start, end, replacement, "planted" or "vote", probability of a read carrying it)]"""
    hi = len(t) if hi is None else hi
    out = []
    p = lo + 8
    while True:
        p += int(rng.integers(0, step))
        if p + 9 >= hi: break
        d = p % W
        if d < GUARD or d > W - GUARD - 2:
            p += 1; continue
        kind = KINDS[rng.integers(len(KINDS))]
        made = pc._site(rng, t, p, kind)
        if made is None:
            p += 1; continue
        (st, en, rep), = made[0]
        out.append((st, en, rep, "planted" if rng.uniform() < 0.25 else "vote", float(rng.uniform(0.15, 0.85))))
        p = made[1] + 7
    for w in {s[0] // W for s in out}:                                       # every window gets a planted backbone error
        if not any(s[3] == "planted" for s in out if s[0] // W == w):
            x = next(i for i, s in enumerate(out) if s[0] // W == w); out[x] = out[x][:3] + ("planted",) + out[x][4:]
    return out


def _apply(t, chosen, s=0, e=None):
    """t[s:e] with the chosen alleles [(start, end, replacement)] applied where they lie at least 7 bases inside"""
    e = len(t) if e is None else e
    x = list(t[s:e])
    for st, en, rep in sorted(chosen, reverse=True):
        if st >= s + 7 and en <= e - 7: x[st - s:en - s] = list(rep)
    return "".join(x)


def _backbone_alleles(rng, sites):
    return [(st, en, rep) for st, en, rep, cls, p in sites if cls == "planted" or rng.uniform() < 0.5]


def _read_alleles(rng, sites):
    return [(st, en, rep) for st, en, rep, cls, p in sites if cls == "vote" and rng.uniform() < p]


def _quals(rng, n, lo=12, hi=42):
    return "".join(chr(33 + int(q)) for q in rng.integers(lo, hi, size=n))


def _cut_to_length(t, alleles, Bl):
    """(n, backbone) with backbone = _apply(t, alleles, 0, n) of exactly Bl bases"""
    for n in sorted(range(Bl - 12, Bl + 13), key=lambda n: abs(n - Bl)):
        if 16 <= n <= len(t):
            b = _apply(t, alleles, 0, n)
            if len(b) == Bl: return n, b
    raise AssertionError("no template length gives a backbone of %d bases" % Bl)


# ---------------------------------------------------------------- (a)
def _group_a(gi, seed):
    Bl = A_LENGTHS[gi % len(A_LENGTHS)]
    rng = _rng(0, gi, seed)
    t = pc._template(rng, Bl + 16)
    sites = _sites(rng, t, 200)
    alle = _backbone_alleles(rng, sites)
    n, bb = _cut_to_length(t, alle, Bl)
    nreads = 3 + gi % 4
    reads = [_apply(t, _read_alleles(rng, sites), 0, n) for _ in range(nreads)]
    quals = [_quals(rng, len(r)) for r in reads]
    return Group("a/%d#%d" % (Bl, gi), bb, reads, quals, BASE, "".join(t[:n]))


# ---------------------------------------------------------------- (b)
def _group_b(gi, seed, variant):
    Bl, W, PAD = 600, 200, 30
    rng = _rng(1, gi, seed)
    t = pc._template(rng, PAD + Bl + 40 + PAD)
    sites = _sites(rng, t, W, lo=PAD, hi=len(t) - PAD, step=12)
    sites = [s for s in sites if GUARD <= (s[0] - PAD) % W <= W - GUARD - 2]            # window edges are counted from the backbone's start
    alle = _backbone_alleles(rng, sites)
    for n in sorted(range(Bl - 30, Bl + 31), key=lambda n: abs(n - Bl)):
        if len(_apply(t, alle, PAD, PAD + n)) == Bl: break
    else: raise AssertionError
    inner = [a for a in alle if a[0] >= PAD + 7 and a[1] <= PAD + n - 7]

    def tp(b):                                                              # template position of backbone coordinate b
        return min(range(PAD, PAD + n + 1), key=lambda p: (abs(p - PAD + sum(len(r) - (e - s) for s, e, r in inner if e <= p) - b), p))
    # A layer of four bases is placed by those four letters alone, and a 4-mer recurs in 200 bases of a template without equal neighbours more often than not
    # (each recurrence a co-optimal placement).  So windows 1 and 2 begin with a doubled base: the one place of the template where two neighbours are equal.
    for w in (1, 2):
        e = tp(w * W)
        t[e + 1] = t[e]
        if t[e + 2] == t[e]: t[e + 2] = pc._others(t[e], t[e + 3])[0]
    # Every sixth group: no layer of window 0 starts within the slack (all are end-free there), and the backbone's last base of window 0 is wrong.  An end-free
    # layer leaves a mismatching last base unaligned (one gap beats one mismatch): it becomes a sink node of its own, and the heaviest of them ends the consensus -
    # the one place where the bases that an alignment leaves outside the graph decide a result.
    # Where the template leaves two other letters for that position, the reads vote there too (template 0.6, the fourth letter 0.4): a later read matches the sink
    # node of an earlier one with its letter, so there is one sink node per letter and the heavier sum wins.
    lead = 2 if gi % 6 == 2 else 0
    edge_alt = None
    if lead:
        e = tp(W) - 1
        o = pc._others(t[e - 1], t[e], t[e + 1])
        alle = alle + [(e, e + 1, o[0])]
        if len(o) > 1: edge_alt = (e, e + 1, o[1])
    bb = _apply(t, alle, PAD, PAD + n)
    assert len(bb) == Bl
    spans = [(tp(lead), PAD + n), (tp(lead + (lead > 0)), PAD + n)]         # two reads over (almost) the whole backbone: every window has its two layers
    d = [int(x) for x in rng.permutation(4)]
    w1, w2 = int(rng.integers(0, 2)), int(rng.integers(1, 3))
    spans.append((tp(max(w1 * W + d[0], lead)), tp((w2 + 1) * W - d[1])))  # begin = d[0] (GLOBAL below 2), end = 199 - d[1] (GLOBAL at 0 only)
    spans.append((tp(W - d[2]), tp(Bl)))                                    # d[2] bases of window 0: a layer below 0.02 W = 4 there (dropped), begin 0 in window 1
    spans.append((tp(lead), tp(2 * W + 3 + gi % 2)))                        # 3 / 4 bases into the last window: dropped / kept
    spans.append((tp(W + d[3]), tp(2 * W + d[1])))
    o1, o2 = int(rng.integers(1, 31)), int(rng.integers(1, 31))
    # overhangs the backbone's ends (every group but each third one: where the aligner puts the overhanging bases is pinned, where the window graph puts them is often a tie)
    if gi % 3 == 0: spans.append((PAD - o1, PAD + n + o2))
    elif gi % 3 == 1: spans.append((PAD - o1, tp(W + 4 - gi % 2)))
    else: spans.append((tp(max(d[0], lead)), tp(W + 4 - gi % 2)))
    reads = [_apply(t, _read_alleles(rng, sites) + ([edge_alt] if edge_alt and rng.uniform() < 0.4 else []), s, e) for s, e in spans]
    quals = [_quals(rng, len(r)) for r in reads]
    prm = dict(BASE, aln_mode=3, trim=3) if variant else dict(BASE)
    return Group("b/%s#%d" % ("mode3trim3" if variant else "mode2trim2", gi), bb, reads, quals, prm, "".join(t[PAD:PAD + n]))


# ---------------------------------------------------------------- (c)
def _template3(rng, n):
    """letters C / G / T only, drawn independently (equal neighbours allowed: two letters per position would make the flanks repeat themselves)"""
    return ["CGT"[rng.integers(3)] for _ in range(n)]


def _sub_sites(rng, t, lo, hi, step=10):
    """substitution sites inside t[lo:hi], C / G / T only, the new letter different from both neighbours"""
    out = []
    p = lo + 8
    while True:
        p += int(rng.integers(0, step))
        if p + 9 >= hi: break
        o = [c for c in "CGT" if c not in (t[p - 1], t[p], t[p + 1])]
        if not o:
            p += 1; continue
        out.append((p, p + 1, o[0], "planted" if rng.uniform() < 0.25 else "vote", float(rng.uniform(0.15, 0.85))))
        p += 8
    return out


C_KINDS = ("q_exact", "q_minus", "q_plus", "fasta", "bang", "span140", "span139", "span141", "span70")


def _group_c(gi, seed):
    rng = _rng(2, gi, seed)
    kind = C_KINDS[gi % len(C_KINDS)]
    W = 200
    if kind.startswith("span"):
        Bl = 100 if kind == "span70" else 200
        want = {"span140": 140, "span139": 139, "span141": 141, "span70": 70}[kind]
        run = Bl - want                                                        # the run of A, which read 1 lacks as a whole (a read that kept some of them could pair them with any)
        flank = (Bl - run) // 2
        for attempt in range(50):
            # redrawn until the aligner's own rules (ed_reference) give read 1 the spans the case is named after: with substitutions in the flanks a shifted
            # flank can cost exactly what the long deletion costs, and the traceback prefers the diagonal
            rng = _rng(2, gi, 1000 * seed + attempt)
            t = _template3(rng, flank) + ["A"] * run + _template3(rng, Bl - flank - run)
            sites = _sub_sites(rng, t, 0, flank) + _sub_sites(rng, t, flank + run, Bl)      # substitutions only: the backbone's length is the span the case is about
            bb = _apply(t, _backbone_alleles(rng, sites))
            reads = [_apply(t, _read_alleles(rng, sites)) for _ in range(4)]
            reads[1] = reads[1][:flank] + reads[1][flank + run:]
            cols = ed.align_pair(reads[1], bb)[2]
            if len(cols) and (cols[0, 0], cols[-1, 0], cols[0, 1], cols[-1, 1]) == (0, want - 1, 0, Bl - 1): break
        else: raise AssertionError("no draw gives the spans (%d, %d)" % (want, Bl))
        quals = [_quals(rng, len(r)) for r in reads]
        return Group("c/%s#%d" % (kind, gi), bb, reads, quals, dict(BASE, k=9, w=12) if kind == "span70" else BASE, "".join(t))
    Bl = 200
    t = pc._template(rng, Bl)
    sites = _sites(rng, t, W)
    bb = _apply(t, [a for a in _backbone_alleles(rng, sites) if len(a[2]) == a[1] - a[0]])
    reads = [_apply(t, _read_alleles(rng, sites)) for _ in range(5)]
    quals = [_quals(rng, len(r)) for r in reads]
    if kind in ("q_exact", "q_minus", "q_plus", "fasta"):
        # reads 1 - 3: quality sums of exactly 10 len, 10 len - 1, 10 len + 1 (the order rotates with the group)
        order = [0, -1, 1]; order = order[gi % 3:] + order[:gi % 3]
        for x, dlt in zip((1, 2, 3), order):
            q = [10] * len(reads[x]); q[len(q) // 2] += dlt
            quals[x] = "".join(chr(33 + v) for v in q)
        if kind == "fasta": quals = None
    else:
        quals[2] = "!" * len(reads[2])                                          # weight 0 on every base: mean quality 0, the layer is dropped
        quals[3] = "".join("!" if i % 2 else "5" for i in range(len(reads[3])))  # every other base weighs nothing; mean quality 10: kept
    return Group("c/%s#%d" % (kind, gi), bb, reads, quals, BASE, "".join(t))


# ---------------------------------------------------------------- (d)
D_KINDS = ("half_rc", "with_n", "one_unrelated", "all_unrelated", "no_reads", "one_read", "short_backbone", "k25", "w_below_k", "chimeric_strands", "half_rc_fasta", "all_rc")


def _group_d(gi, seed):
    rng = _rng(3, gi, seed)
    kind = D_KINDS[gi % len(D_KINDS)]
    W = 200
    Bl = (230, 300, 405)[gi % 3]
    prm = dict(BASE)
    if kind == "short_backbone":
        t = pc._template(rng, 10); bb = "".join(t)
        reads = ["".join(t)] * 3; quals = [_quals(rng, 10) for _ in reads]
        return Group("d/%s#%d" % (kind, gi), bb, reads, quals, prm, bb)
    t = pc._template(rng, Bl + 16)
    sites = _sites(rng, t, W)
    alle = _backbone_alleles(rng, sites)
    n, bb = _cut_to_length(t, alle, Bl)
    nreads = {"no_reads": 0, "one_read": 1}.get(kind, 4 + gi % 3)
    reads = [_apply(t, _read_alleles(rng, sites), 0, n) for _ in range(nreads)]
    if kind == "with_n":
        for x in (1, 2):
            r = list(reads[x])
            for p in rng.choice(np.arange(20, len(r) - 20), size=3, replace=False): r[int(p)] = "N"
            reads[x] = "".join(r)
    if kind == "one_unrelated": reads[1] = "".join(pc._template(rng, Bl))
    if kind == "all_unrelated": reads = ["".join(pc._template(rng, Bl - x)) for x in range(nreads)]
    if kind == "chimeric_strands":
        # forward part, reverse-complement part: the first split point (from the middle outwards) at which the strand rule itself counts a == b > 0, if there is one
        fwd, rev = set(ref.minimizers(bb, 13, 20)), set(ref.minimizers(ref.revcomp(bb), 13, 20))
        mid = len(reads[2]) // 2
        # (and, failing that, with up to 30 bases cut from the end of the second part)
        found = None
        for cut in range(0, 31):
            for h in sorted(range(40, len(reads[2]) - 70), key=lambda h: (abs(h - mid), h)):
                r = reads[2][:h] + ref.revcomp(reads[2][h:len(reads[2]) - cut])
                a, b, _ = ref.strand_call(r, fwd, rev, 13, 20)
                if a == b > 0:
                    found = r; break
            if found: break
        reads[2] = found or reads[2][:mid] + ref.revcomp(reads[2][mid:])
    quals = [_quals(rng, len(r)) for r in reads]
    if kind in ("half_rc", "half_rc_fasta", "with_n", "k25", "w_below_k", "one_unrelated", "chimeric_strands"):
        for x in range(0, len(reads), 2):
            if kind == "chimeric_strands" and x == 2: continue                # the minimizers of a reverse complement are not those of the read: its a == b would be lost
            reads[x] = ref.revcomp(reads[x]); quals[x] = quals[x][::-1]
    if kind == "all_rc":
        reads = [ref.revcomp(r) for r in reads]; quals = [q[::-1] for q in quals]
    if kind == "half_rc_fasta": quals = None
    if kind == "k25": prm.update(k=25, w=30)
    if kind == "w_below_k": prm.update(k=15, w=10)
    return Group("d/%s#%d" % (kind, gi), bb, reads, quals, prm, "".join(t[:n]))


# ---------------------------------------------------------------- (e)
def _group_e(gi, seed, trim):
    rng = _rng(4, gi, seed)
    W = 500
    total = 3000 if gi % 2 == 0 else 3003                                    # mean read length exactly 1000 (not TGS) / 1001 (TGS)
    short = [(int(rng.integers(5, 41)), int(rng.integers(5, 41))) for _ in range(2)] + [(int(rng.integers(5, 41)), int(rng.integers(18, 28)))]
    n = (total + sum(a + b for a, b in short)) // 3 + 2
    t = pc._template(rng, n + 16)
    sites = _sites(rng, t, W, lo=45, hi=n - 45, step=24)
    alle = _backbone_alleles(rng, sites)
    bb = _apply(t, alle, 0, n)
    reads = []
    for a, b in short: reads.append(_apply(t, _read_alleles(rng, sites), a, n - b))
    # the third read is cut or extended at its far end so that the total is exact (it still stops 5 - 40 bases short)
    fix = total - sum(len(r) for r in reads)
    b = short[2][1]
    if fix > 0: reads[2] = reads[2] + "".join(t[n - b:n - b + fix])
    elif fix < 0: reads[2] = reads[2][:fix]
    assert sum(len(r) for r in reads) == total and 5 <= b - fix <= 40, (fix, b)
    quals = [_quals(rng, len(r)) for r in reads]
    return Group("e/%s/trim%d#%d" % ("tgs" if total == 3003 else "ngs", trim, gi), bb, reads, quals, dict(BASE, window=W, trim=trim, iters=1), "".join(t[:n]))


# ---------------------------------------------------------------- (f)
def _group_f(gi, seed):
    rng = _rng(5, gi, seed)
    W = 200
    Bl = 418 + gi % 5                                                         # the backbone
    Tl = (419, 421, 420, 418, 422, 421, 419)[gi % 7]                          # the template the reads come from: Tl - 400 below / at / above W / 10 = 20
    t = pc._template(rng, Tl)
    sites = [s for s in _sites(rng, t, W, hi=400 - GUARD) if s[3] == "vote"]
    # planted indels: single bases inserted into / deleted from the backbone, GUARD away from window edges and sites
    taken = [s[0] for s in sites]
    alle = [(s[0], s[1], s[2]) for s in sites if rng.uniform() < 0.5]
    need = Bl - (Tl + sum(len(r) - (e - s) for s, e, r in alle))
    tries = 0
    while need != 0 and tries < 4000:
        tries += 1
        p = int(rng.integers(20, 380))
        if not (GUARD + 4 <= p % W <= W - GUARD - 6) or any(abs(p - x) < 9 for x in taken): continue
        made = pc._site(rng, t, p, "ins" if need > 0 else "del")
        if made is None: continue
        alle.append(made[0][0]); taken.append(p); need += -1 if need > 0 else 1
    bb = _apply(t, alle)
    assert len(bb) == Bl, (len(bb), Bl)
    reads = [_apply(t, _read_alleles(rng, sites)) for _ in range(4 + gi % 3)]
    quals = [_quals(rng, len(r)) for r in reads]
    return Group("f/%d_from_%d#%d" % (Tl, Bl, gi), bb, reads, quals, dict(BASE, iters=3), "".join(t))


N_GROUPS = {"a_geometry": 13, "b_edges": 12, "c_filters": 18, "d_strands": 24, "e_trim": 4, "f_iterations": 14}
_families = {}


def family(name):
    """the groups of a family (built once)"""
    if name not in _families:
        n = N_GROUPS[name]; sd = lambda gi: SEEDS.get((name, gi), gi)
        if name == "a_geometry": gs = [_group_a(gi, sd(gi)) for gi in range(n)]
        elif name == "b_edges": gs = [_group_b(gi, sd(gi), v) for gi in range(n) for v in (0, 1)]
        elif name == "c_filters": gs = [_group_c(gi, sd(gi)) for gi in range(n)]
        elif name == "d_strands": gs = [_group_d(gi, sd(gi)) for gi in range(n)]
        elif name == "e_trim": gs = [_group_e(gi, sd(gi), trim) for gi in range(n) for trim in (0, 1, 2, 3)]
        else: gs = [_group_f(gi, sd(gi)) for gi in range(n)]
        _families[name] = gs
    return _families[name]


FAMILIES = tuple(sorted(N_GROUPS))
_expected = {}


def expected(name, subgraph=False):
    """[(seqs, used, aln, decided, info)] of a family by the reference, computed once and handed out read-only; subgraph: under NGSID_ALN_SUBGRAPH"""
    if (name, subgraph) not in _expected:
        out = []
        for g in family(name):
            r = ref.polish_reference(g.backbone, g.reads, g.quals, subgraph=subgraph, **g.prm)
            for a in r[2]: a.setflags(write=False)
            out.append(r)
        _expected[(name, subgraph)] = out
    return _expected[(name, subgraph)]


# ---------------------------------------------------------------- calls: one group, or all groups of a family that share their parameters
def call_keys(name):
    """the distinct (parameters, FASTA or FASTQ) of a family, each with the indices of its groups: one library call takes one set of parameters and one kind of reads"""
    keys = {}
    for x, g in enumerate(family(name)):
        keys.setdefault((tuple(sorted(g.prm.items())), g.quals is None), []).append(x)
    return sorted(keys.items())


def pack(groups, shuffle_seed=None):
    """the arguments of ONE call over `groups` -> (backbones, reads, quals or None, read_order (uint32) or None, grp_off (uint64), listed: the groups' positions in call order).
    shuffle_seed: reads are stored in a shuffled order and reached through read_order, groups are listed in a shuffled order."""
    flat = [(gi, k) for gi, g in enumerate(groups) for k in range(len(g.reads))]
    if shuffle_seed is None:
        store = list(range(len(flat))); listed = list(range(len(groups)))
    else:
        rng = np.random.default_rng([91, shuffle_seed])
        store = [int(x) for x in rng.permutation(len(flat))]; listed = [int(x) for x in rng.permutation(len(groups))]
    slot_of = {flat[f]: x for x, f in enumerate(store)}
    fasta = all(g.quals is None for g in groups)
    reads = [groups[flat[f][0]].reads[flat[f][1]] for f in store]
    quals = None if fasta else [groups[flat[f][0]].quals[flat[f][1]] for f in store]
    order, off = [], [0]
    for gi in listed:
        order += [slot_of[(gi, k)] for k in range(len(groups[gi].reads))]; off.append(len(order))
    return ([groups[gi].backbone for gi in listed], reads, quals, None if shuffle_seed is None else np.array(order, dtype=np.uint32), np.array(off, dtype=np.uint64), listed)


def differences(exp, seqs, used, aln=None, last_only=False):
    """what one group's output (seqs[it], used[it], aln[it] = records of its listed reads, or None) has that the reference's (an entry of expected()) has not, as text;
    last_only: seqs / used hold the last iteration alone (ngsid_polish)"""
    e_seqs, e_used, e_aln = exp[0], exp[1], exp[2]
    if last_only: e_seqs, e_used, e_aln = e_seqs[-1:], e_used[-1:], e_aln[-1:]
    out = []
    for it in range(len(e_seqs)):
        if seqs[it] != e_seqs[it]: out.append("iteration %d sequence\n  got      %s\n  expected %s" % (it, seqs[it], e_seqs[it]))
        if int(used[it]) != e_used[it]: out.append("iteration %d n_used: got %d, expected %d" % (it, int(used[it]), e_used[it]))
        if aln is not None and not np.array_equal(np.asarray(aln[it]), e_aln[it]):
            out.append("iteration %d records\n  got      %s\n  expected %s" % (it, np.asarray(aln[it]).tolist(), e_aln[it].tolist()))
    return out
