"""Deterministic POA groups (fixed seeds) for the reference anchor: tests/test_poa_reference_cpu.py and tests/test_gpu_poa_reference.py.

A group = reads of one template that differ from it only at VARIANT SITES, so that the consensus is a set of real votes decided by the weights and an
independent reference rarely has to break a tie (poa_reference.py reports when it did):
  - the template has no two equal neighbouring bases;
  - sites are at least 7 bases apart and at least 7 bases from the ends of any read;
  - a site has one fixed set of alleles, drawn per read with per-site probabilities;
  - kinds: "del" one base deleted (only where its two neighbours differ); "ins" a base inserted that differs from both neighbours; "sub" a base
    substituted by one that differs from both neighbours; "sub3" the same with three alleles (the template is redrawn there so that the two neighbours
    are equal, which leaves two other letters); "nest2" / "nest3" deletions of 1 and 2 (and 3) bases that END at the same node, redrawn until neither
    flank of a deletion equals one of its deleted bases (else the gaps could be split around a match: a tie) - 3 and 4 in-edges at one node;
  - qualities are random phred 2..41;
  - reads other than the first are clipped by 0..25 bases per end where the family says so (LOCAL, SEMI); templates under 200 bases are clipped by at
    most an eighth of their length, so that sites still fit between the clipped ends.
One more family clips the first read as well: overhanging heads and tails of later reads become new branches.

Shapes are the smallest at which the engine can still go wrong: template lengths around each band width (63 64 65 / 127 128 129 / 255 257), templates
longer than the band so that it slides (400 at 64 columns, 1000 at 128), depths 2 3 5 10 24 40, one shallow-template deep group (150 x 80).  Two groups
of 1000 x 40 in the whole file.  Every family's groups come in three chunks ("small", "mid", "long") so that no test waits for more than a few seconds
of reference time.
"""
import numpy as np
import poa_reference as ref

LOCAL, GLOBAL, SEMI = ref.LOCAL, ref.GLOBAL, ref.SEMI
ACGT = "ACGT"
INDELS = ("del", "ins", "nest2", "nest3")
ALL_KINDS = ("del", "ins", "sub", "sub3", "nest2", "nest3")
WEIGHTS = (0, 1, 2, 3, 7, 50, 1000, (1 << 20) - 1, 1 << 20, (1 << 20) + 5)

#            template, depth, band
SMALL = [(63, 5, 64), (64, 3, 64), (65, 2, 64), (63, 10, 64), (64, 24, 64), (127, 5, 128), (128, 10, 128), (129, 3, 128), (128, 40, 128), (65, 5, 64)]
MID = [(255, 5, 256), (257, 10, 256), (255, 3, 256), (150, 10, 64), (150, 24, 64), (400, 24, 64), (400, 5, 64), (257, 2, 256)]
CHUNKS = ("small", "mid", "long")


class Group:
    def __init__(self, name, template, seqs, quals, weights, band):
        self.name, self.template, self.seqs, self.quals, self.weights, self.band = name, template, seqs, quals, weights, band


class Family:
    def __init__(self, fid, name, mode, scores, kinds, clipped=False, fasta=False, weighted=False, long=((1000, 5, 128),), clip_first=False):
        self.fid, self.name, self.mode, self.kinds, self.clipped, self.fasta, self.weighted = fid, name, mode, kinds, clipped, fasta, weighted
        self.clip_first = clip_first
        self.match, self.mismatch, self.gap = scores
        self.shapes = {"small": SMALL, "mid": MID, "long": list(long)}
        self._groups = {}

    def groups(self, chunk):
        if chunk not in self._groups:
            self._groups[chunk] = [make_group(self, CHUNKS.index(chunk) * 100 + i, *shape) for i, shape in enumerate(self.shapes[chunk])]
        return self._groups[chunk]

    def all_groups(self):
        return [g for c in CHUNKS for g in self.groups(c)]


FAMILIES = {f.name: f for f in [
    Family(0, "local_542_indels", LOCAL, (5, -4, -2), INDELS, clipped=True, long=((1000, 5, 128), (150, 80, 64))),
    Family(1, "local_532_all", LOCAL, (5, -3, -2), ALL_KINDS, clipped=True, long=((1000, 40, 128),)),
    Family(2, "global_354_all", GLOBAL, (3, -5, -4), ALL_KINDS, long=((1000, 40, 128),)),
    Family(3, "semi_354_clipped", SEMI, (3, -5, -4), ALL_KINDS, clipped=True),
    Family(4, "fasta_local_542", LOCAL, (5, -4, -2), INDELS, clipped=True, fasta=True),
    Family(5, "weighted_global_354", GLOBAL, (3, -5, -4), ALL_KINDS, weighted=True),
    Family(6, "weighted_local_532", LOCAL, (5, -3, -2), ALL_KINDS, clipped=True, weighted=True),
    # beyond the seven families above: the FIRST read is clipped too, so the heads and tails of later reads hang over the graph and become new branches
    # (several sources and sinks) - what clipped copies of a full-length first read never do
    Family(7, "local_532_short_first", LOCAL, (5, -3, -2), ALL_KINDS, clipped=True, clip_first=True),
]}


def _template(rng, n):
    t = [ACGT[rng.integers(4)]]
    while len(t) < n:
        c = ACGT[rng.integers(4)]
        if c != t[-1]: t.append(c)
    return t


def _redraw(rng, t, lo, hi, ok):
    """redraw t[lo:hi] until no two neighbours (the flanks included) are equal and ok(t) holds"""
    for _ in range(2000):
        for x in range(lo, hi): t[x] = ACGT[rng.integers(4)]
        if all(t[x] != t[x + 1] for x in range(lo - 1, hi)) and ok(t): return True
    return False


def _others(*used):
    return [c for c in ACGT if c not in used]


def _site(rng, t, p, kind):
    """-> (alleles, next free position) with alleles = [(start, end, replacement)] (the template's own allele is not listed), or None.
    The site touches template positions [p, next free position)."""
    if kind == "del":
        return ([(p, p + 1, "")], p + 1) if t[p - 1] != t[p + 1] else None
    if kind == "ins":
        o = _others(t[p], t[p + 1])
        return [(p + 1, p + 1, o[rng.integers(len(o))])], p + 1
    if kind == "sub":
        o = _others(t[p - 1], t[p], t[p + 1])
        return [(p, p + 1, o[rng.integers(len(o))])], p + 1
    if kind == "sub3":
        if not _redraw(rng, t, p - 1, p + 2, lambda t: t[p - 1] == t[p + 1]): return None
        o = _others(t[p - 1], t[p])
        return [(p, p + 1, o[0]), (p, p + 1, o[1])], p + 2
    k = 2 if kind == "nest2" else 3
    e = p + k + 1                                             # the deletions remove t[e-d:e], d = 1..k, and all end at node e

    def ok(t):
        # deleting t[s:e], s = e - d, costs d gaps wherever they go: the left flank t[s-1] must equal none of the deleted bases (else it matches there and the
        # gaps split around it), neither must the right flank t[e], and the deletion joins different bases.  With four letters the last demand cannot hold
        # for d = 3 (t[e-3:e] and t[e] are four different letters and t[e-4] equals none of the first three): that deletion joins two equal bases,
        # which shifts nothing because every other base of the window differs from them.
        for d in range(1, k + 1):
            s = e - d
            if any(t[s - 1] == t[s - 1 + x] or t[e] == t[e - x] for x in range(1, d + 1)): return False
            if d < 3 and t[s - 1] == t[e]: return False
        return True
    if not _redraw(rng, t, p, e + 1, ok): return None
    return [(e - d, e, "") for d in range(1, k + 1)], e + 1


def make_group(fam, gi, n, depth, band):
    rng = np.random.default_rng([20240607, fam.fid, gi, n, depth])
    clip = (25 if n >= 200 else n // 8) if fam.clipped else 0
    t = _template(rng, n)
    sites = []
    p = clip + 7 + 1
    step = max(4, n // 12)
    while True:
        p += int(rng.integers(0, step))
        if p + 6 + 7 + clip >= n: break
        kind = fam.kinds[rng.integers(len(fam.kinds))]
        if depth < 5 and kind in ("nest2", "nest3", "sub3"):      # too few reads to see three or four alleles
            two = [x for x in fam.kinds if x in ("del", "ins", "sub")]; kind = two[rng.integers(len(two))]
        made = _site(rng, t, p, kind)
        if made is None:
            p += 1; continue
        alleles, nxt = made
        if len(alleles) == 1: pr = [1.0 - rng.uniform(0.4, 0.85)]; pr.append(1.0 - pr[0])
        else:
            pr = rng.dirichlet([1.0] + [1.5] * len(alleles)).tolist()
        sites.append((alleles, np.cumsum(pr)))
        p = nxt + 7
    assert all(t[x] != t[x + 1] for x in range(n - 1))
    template = "".join(t)
    seqs, quals = [], []
    for k in range(depth):
        s = template
        for alleles, cum in reversed(sites):
            a = int(np.searchsorted(cum, rng.uniform(), side="right"))
            if a >= 1 and a <= len(alleles):
                st, en, rep = alleles[a - 1]; s = s[:st] + rep + s[en:]
        if (k or fam.clip_first) and clip:
            a, b = int(rng.integers(0, clip + 1)), int(rng.integers(0, clip + 1)); s = s[a:len(s) - b]
        seqs.append(s)
        quals.append("".join(chr(33 + int(q)) for q in rng.integers(2, 42, size=len(s))))
    weights = None
    if fam.weighted:
        weights = [int(WEIGHTS[rng.integers(len(WEIGHTS))]) for _ in range(depth)]; quals = None
    elif fam.fasta: quals = None
    return Group("%s/%dx%d#%d" % (fam.name, n, depth, gi), template, seqs, quals, weights, band)


_expected = {}


def expected(fam, chunk):
    """[(consensus, cov, decided)] of a family's chunk by the reference, computed once"""
    key = (fam.name, chunk)
    if key not in _expected:
        _expected[key] = [ref.poa_reference(g.seqs, g.quals, g.weights, fam.mode, fam.match, fam.mismatch, fam.gap) for g in fam.groups(chunk)]
    return _expected[key]
