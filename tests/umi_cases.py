"""Generators of the UMI tests - test infrastructure, not a test: sets of short sequences that exercise the seeded search, and reads of molecules with a random UMI
pair.  Everything is seeded."""
import numpy as np
import variants_cases as vc
import demux_reference as dr

# a design with four 20-letter flanks, any two (and any one against another's reverse complement) at least 8 edits apart
FLANKS = tuple(dr.make_tags(4, length=20, min_dist=8, seed=17))
UMI_LEN, LEN_SLACK = 18, 2


def edit_inside(rng, s, k, margin=4):
    """k random edits (substitution, insertion, deletion) at least `margin` letters away from both ends of s"""
    s = list(s)
    for _ in range(k):
        p = int(rng.integers(margin, len(s) - margin)); kind = int(rng.integers(0, 3))
        if kind == 0: s[p] = "ACGT"[("ACGT".index(s[p]) + int(rng.integers(1, 4))) % 4]
        elif kind == 1: s.insert(p, "ACGT"[int(rng.integers(0, 4))])
        else: del s[p]
    return "".join(s)


def one_edit(rng, s):
    """exactly one edit anywhere in s"""
    s = list(s); p = int(rng.integers(0, len(s))); kind = int(rng.integers(0, 3))
    if kind == 0: s[p] = "ACGT"[("ACGT".index(s[p]) + int(rng.integers(1, 4))) % 4] if s[p] in "ACGT" else "A"
    elif kind == 1: s.insert(p, "ACGT"[int(rng.integers(0, 4))])
    else: del s[p]
    return "".join(s)


def make_run(seed, n_templates=3, length=300, molecules=8, reads=6, error=0.004, rc_fraction=0.3, n_no_flank=3, n_bad_len=3, flanks=FLANKS):
    """n_templates random templates x `molecules` molecules each, every molecule with a random UMI pair and `reads` reads:
    junk + fwd_pre' + u_fwd' + fwd_post' + noisy template + revcomp(rev_pre' + u_rev' + rev_post') + junk, flanks with 0 .. 2 interior edits, at most ONE edit in the
    two UMIs of a read together, rc_fraction of the reads reverse-complemented as a whole; + n_no_flank reads whose forward flanks are random letters and n_bad_len
    reads whose forward UMI has UMI_LEN + LEN_SLACK + 3 letters.  Shuffled.
    -> dict(seqs, quals, names, molecule [n] (-1: none), strand [n], templates, template_of [molecules], umis [(u_fwd, u_rev)])"""
    rng = np.random.default_rng(seed)
    fp, fq, rp, rq = flanks
    templates = [vc.rand_seq(rng, length) for _ in range(n_templates)]
    umis, template_of, rows = [], [], []
    junk = lambda: vc.rand_seq(rng, int(rng.integers(0, 11)))

    def read_of(t, uf, ur, head_flanks=True):
        a, b = (edit_inside(rng, fp, int(rng.integers(0, 3))), edit_inside(rng, fq, int(rng.integers(0, 3)))) if head_flanks else (vc.rand_seq(rng, len(fp)), vc.rand_seq(rng, len(fq)))
        tail = edit_inside(rng, rp, int(rng.integers(0, 3))) + ur + edit_inside(rng, rq, int(rng.integers(0, 3)))
        return junk() + a + uf + b + vc.mutate(rng, templates[t], error) + dr.revcomp(tail) + junk()

    for t in range(n_templates):
        for _ in range(molecules):
            uf, ur = vc.rand_seq(rng, UMI_LEN), vc.rand_seq(rng, UMI_LEN)
            m = len(umis); umis.append((uf, ur)); template_of.append(t)
            for _ in range(reads):
                f, r = uf, ur
                which = int(rng.integers(0, 3))                         # no edit, one in the forward UMI, one in the reverse UMI
                if which == 1: f = one_edit(rng, uf)
                elif which == 2: r = one_edit(rng, ur)
                rows.append((read_of(t, f, r), m))
    for _ in range(n_no_flank):
        rows.append((read_of(0, vc.rand_seq(rng, UMI_LEN), vc.rand_seq(rng, UMI_LEN), head_flanks=False), -1))
    for _ in range(n_bad_len):
        rows.append((read_of(0, vc.rand_seq(rng, UMI_LEN + LEN_SLACK + 3), vc.rand_seq(rng, UMI_LEN)), -1))
    out = []
    for s, m in rows:
        st = int(rng.random() < rc_fraction)
        out.append((dr.revcomp(s) if st else s, m, st))
    out = [out[i] for i in rng.permutation(len(out))]
    return dict(seqs=[o[0] for o in out], quals=["I" * len(o[0]) for o in out], names=["read%d" % i for i in range(len(out))],
                molecule=np.array([o[1] for o in out]), strand=np.array([o[2] for o in out]), templates=templates, template_of=template_of, umis=umis)


def search_set(rng, d, g):
    """about 200 sequences for one (max_dist, seed_len): the border lengths mixed, pairs whose only intact seed is the last one shifted by +d / -d, or seed 0, pairs at
    exactly d and d + 1, seeds with N, families that match in every seed, substrings at the edges of a sequence"""
    need = (d + 1) * g
    seqs = []
    for L in sorted({0, 1, max(need - 1, 0), min(need, 64), 63, 64}):
        L = min(L, 64)
        a = vc.rand_seq(rng, L, "ACGTN")
        seqs += [a, a, vc.mutate(rng, a, 0.05)[:64], vc.rand_seq(rng, L)]
    if need <= 64:
        L = max(need, min(40, 64 - d))
        seed_at = lambda j: (j * g, (j + 1) * g)
        # one edit in every seed but `keep` (a substitution by a letter the sequence does not hold), so that seed is the only witness; then d leading insertions / deletions
        for keep in (d, 0):
            a = vc.rand_seq(rng, L, "AC")
            b = list(a)
            for j in range(d + 1):
                if j != keep: b[seed_at(j)[0] + g // 2] = "G"
            b = "".join(b)
            seqs += [a, b]                                              # d substitutions: distance exactly d, one intact seed
            if L - 1 >= need: seqs.append(b[:L - 1] + "T")             # d + 1 substitutions, the last one behind the seeds
        a = vc.rand_seq(rng, L, "AC")
        # one insertion (deletion) inside every seed but the last: the last seed is the only intact one, shifted by +d (-d)
        ins, dele = list(a), list(a)
        for j in reversed(range(d)):
            ins.insert(j * g + g // 2, "GT"[j % 2]); del dele[j * g + g // 2]
        seqs.append("".join(dele))
        if L + d <= 64: seqs.append("".join(ins))
        seqs += [a, a[d:]]                                              # the whole of a shifted by -d ...
        if L + d <= 64: seqs += [vc.rand_seq(rng, d, "GT") + a, vc.rand_seq(rng, d, "GT") + a[:L - 1]]      # ... and by +d; +d and one more edit
        # a substring of the query that would start before 0 or end behind the sequence: b is a without its first / last letters
        a = vc.rand_seq(rng, min(need + d, 64), "ACGT")
        seqs += [a, a[1:], a[:-1], a[d:], a[:len(a) - d]]
        # N inside seeds, equal only to N
        a = list(vc.rand_seq(rng, L)); a[g // 2] = "N"; a[g + 1] = "N"
        b = list(a); b[g // 2] = "A"
        seqs += ["".join(a), "".join(b), "".join(a)]
        # a family that matches in every seed: identical copies and copies with a tail edit
        a = vc.rand_seq(rng, min(need + 2, 64))
        seqs += [a] * 6 + [a[:-1] + ("A" if a[-1] != "A" else "C")] * 3
    for k in (d, d + 1):                                                # exactly d and d + 1 apart, at a length that may or may not be seedable
        for n in (36, 64):
            if k <= n: seqs += list(vc.at_distance(rng, n, k))
    while len(seqs) < 200:                                              # related families at 5 %
        root = vc.rand_seq(rng, int(rng.integers(30, 65)))
        seqs += [vc.mutate(rng, root, 0.05)[:64] for _ in range(5)]
    return [seqs[i] for i in rng.permutation(len(seqs))]
