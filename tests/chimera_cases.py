"""Sequences for the chimera tests (tests/test_chimera_cpu.py, tests/test_gpu_chimera.py) and the sweep (tools/chimera_sweep.py): random strings, mutated copies,
families of a given pairwise divergence, two-parent chimeras."""
import numpy as np

ALPHABET = "ACGT"


def rand_seq(rng, n, alphabet=ALPHABET):
    return "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), n))


def mutate(rng, s, rate):
    """substitutions, insertions and deletions, each at rate / 3 per base"""
    out = []
    for c in s:
        u = rng.random()
        if u < rate / 3:
            out.append(ALPHABET[(ALPHABET.index(c) + int(rng.integers(1, 4))) % 4] if c in ALPHABET else "A")
        elif u < 2 * rate / 3:
            out.append(c); out.append(ALPHABET[int(rng.integers(0, 4))])
        elif u < rate:
            continue
        else:
            out.append(c)
    return "".join(out)


def family(rng, n, length, divergence):
    """n sequences of about `length` bases, each `divergence / 2` away from a common root: pairwise divergence about `divergence`"""
    root = rand_seq(rng, length)
    return [mutate(rng, root, divergence / 2) for _ in range(n)]


def chimera_of(a, b, frac):
    """head of a up to frac of its length, tail of b from the same relative position -> (sequence, crossover)"""
    k = int(round(frac * len(a)))
    kb = int(round(frac * len(b)))
    return a[:k] + b[kb:], k


def related(rng, n, m, count):
    """a query of n bases and `count` parents of m bases that share stretches with it"""
    base = rand_seq(rng, max(n, m) + 8)
    q = base[:n]
    parents = []
    for x in range(count):
        s = mutate(rng, base, 0.06 * (x + 1)) + rand_seq(rng, m)
        if x == 1 and m > 4:
            s = rand_seq(rng, m // 2) + s[m // 2:]             # shares the tail only
        parents.append(s[:m])
    return q, parents


def random_small(rng, n_queries, max_len=12, max_pairs=6):
    """-> (queries, parents, pair_off, pair_parent, pair_gid): strings of 0 .. max_len letters over a two- or a four-letter alphabet, gids from {0, 1, 2}"""
    queries, parents, pair_off, pair_parent, gid = [], [], [0], [], []
    for x in range(n_queries):
        alpha = "AC" if x % 2 else ALPHABET
        queries.append(rand_seq(rng, int(rng.integers(0, max_len + 1)), alpha))
        P = int(rng.integers(0, max_pairs + 1))
        for _ in range(P):
            if parents and rng.random() < 0.3:
                pair_parent.append(int(rng.integers(0, len(parents))))
            else:
                pair_parent.append(len(parents)); parents.append(rand_seq(rng, int(rng.integers(0, max_len + 1)), alpha))
            gid.append(int(rng.integers(0, 3)))
        pair_off.append(len(pair_parent))
    if not parents: parents.append("")
    return queries, parents, pair_off, pair_parent, np.asarray(gid, dtype=np.int32)
