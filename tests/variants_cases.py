"""Generators of the variant tests: families at a given divergence, pairs at an exactly known distance, indel-only pairs.  Everything is seeded."""
import numpy as np

BASES = "ACGT"


def rand_seq(rng, n, alphabet=BASES):
    return "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), n))


def mutate(rng, s, rate):
    """every base independently substituted, deleted or followed by an insertion, each with probability rate / 3"""
    out = []
    for ch in s:
        u = rng.random()
        if u < rate / 3: out.append(BASES[(BASES.index(ch) + int(rng.integers(1, 4))) % 4] if ch in BASES else "A")
        elif u < 2 * rate / 3: pass
        elif u < rate: out.append(ch); out.append(BASES[int(rng.integers(0, 4))])
        else: out.append(ch)
    return "".join(out)


def families(rng, n_families, per_family, length, divergence, between=None):
    """n_families random roots (or roots `between` apart from the first), per_family members each at `divergence` from the root, dealt round robin
    -> (sequences, family of each)"""
    roots = [rand_seq(rng, length)]
    for _ in range(1, n_families):
        roots.append(rand_seq(rng, length) if between is None else mutate(rng, roots[0], between))
    seqs, fam = [], []
    for m in range(per_family):
        for f, r in enumerate(roots):
            seqs.append(r if m == 0 else mutate(rng, r, divergence)); fam.append(f)
    return seqs, fam


def at_distance(rng, n, k):
    """a pair of n-base sequences at edit distance exactly k <= n: a is all of A / C, b differs from it at k positions by a letter of G / T.  a holds none of
    those, so each of them costs one edit in any alignment, and k substitutions reach b"""
    a = rand_seq(rng, n, "AC")
    pos = rng.choice(n, size=k, replace=False) if k else []
    b = list(a)
    for p in pos: b[int(p)] = "GT"[int(rng.integers(0, 2))]
    return a, "".join(b)


def indel_only(rng, n, k, where):
    """a (n bases over A/C) and b = a with k letters of G/T inserted in one run: at the start ('lead'), at the end ('trail') or in the middle ('mid').
    ed(a, b) = k (the lengths differ by k, and deleting the run reaches a); the optimal path runs k diagonals off the main one from the run on"""
    a = rand_seq(rng, n, "AC")
    run = rand_seq(rng, k, "GT")
    at = {"lead": 0, "trail": n, "mid": n // 2}[where]
    return a, a[:at] + run + a[at:]


LENGTHS = lambda K: sorted({0, 1, 2, K, K + 1, 2 * K + 1, 63, 64, 65, 127, 128, 129})


def related_pair(rng, la, lb, edits):
    """a of la bases and b of lb bases, b made from a by |lb - la| indels at random places and up to `edits` substitutions: close when the lengths are"""
    a = rand_seq(rng, la)
    b = list(a)
    while len(b) > lb: del b[int(rng.integers(0, len(b)))]
    while len(b) < lb: b.insert(int(rng.integers(0, len(b) + 1)), BASES[int(rng.integers(0, 4))])
    for _ in range(edits):
        if b: b[int(rng.integers(0, len(b)))] = BASES[int(rng.integers(0, 4))]
    return a, "".join(b)
