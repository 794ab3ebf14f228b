"""Case builders for ngsid_recruit, shared by tests/test_recruit_cpu.py (the reference against the host locator) and tests/test_gpu_recruit.py (the kernel against the
reference) - test infrastructure, not a test.

A case is dict(reads, read_off, cons, cons_off, max_ed, both): the arguments of Api.recruit.  build(name) makes it, expected(name) is the reference's hit array; both
are computed once per process."""
import functools
import numpy as np
import recruit_reference as ref

INSTANCE_WORDS = (1, 2, 4, 8, 12, 16, 24, 32)                            # RC_INSTANCES of k_recruit.hip
CHUNK = 128                                                              # RC_CHUNK: letters staged at a time
# 1, 2, around the first two word boundaries, the top of every instance and one letter beyond (the next instance is taken), the longest consensus
PATTERN_LENGTHS = sorted({1, 2, 63, 64, 65, 127, 128, 129} | {64 * w for w in INSTANCE_WORDS} | {64 * w + 1 for w in INSTANCE_WORDS[:-1]})


def rand(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def substitute(s, positions):
    """another letter at every position that exists"""
    t = list(s)
    for p in positions:
        if 0 <= p < len(t):
            t[p] = "ACGT"[("ACGT".index(t[p]) + 1) % 4] if t[p] in "ACGT" else "A"
    return "".join(t)


def noisy(rng, s, rate):
    """substitutions, insertions and deletions at `rate` per letter"""
    out = []
    for c in s:
        u = rng.random()
        if u < rate / 3:
            continue                                                    # a deletion
        if u < 2 * rate / 3:
            out.append(rand(rng, 1))                                    # an insertion in front of the letter
        out.append(substitute(c, [0]) if 2 * rate / 3 <= u < rate else c)
    return "".join(out)


def _case(groups, both=True):
    """groups: [(reads, consensuses, max_ed per consensus)]"""
    reads, cons, max_ed, read_off, cons_off = [], [], [], [0], [0]
    for r, c, k in groups:
        assert len(c) == len(k)
        reads += r; cons += c; max_ed += [int(x) for x in k]
        read_off.append(len(reads)); cons_off.append(len(cons))
    return dict(reads=reads, read_off=np.array(read_off, dtype=np.uint64), cons=cons, cons_off=np.array(cons_off, dtype=np.uint64),
                max_ed=np.array(max_ed, dtype=np.int32), both=both)


def _pattern_lengths():
    """one group per length: the pattern and a variant of it three substitutions away; a read that holds the pattern exactly, one with edits in the last rows of a block
    and the first rows of the next, one with a run of deletions and one with a run of insertions across a block boundary; every second read on the other strand"""
    rng = np.random.default_rng(101)
    groups = []
    for m in PATTERN_LENGTHS:
        p = rand(rng, m)
        variant = substitute(p, [m // 3, m // 2, m - 1])
        bounds = sorted({64, 64 * ((m - 1) // 64)} - {0}) if m > 64 else [m]      # the first and the last block boundary inside the pattern
        edits = [b + d for b in bounds for d in (-2, -1, 0, 1)]
        b0 = bounds[0]
        bodies = [p, substitute(p, edits), p[:max(b0 - 3, 0)] + p[b0 + 3:], p[:b0 - 1] + rand(rng, 5) + p[b0 - 1:]]
        reads = [rand(rng, 20) + body + rand(rng, 15) for body in bodies]
        reads = [ref.revcomp(r) if x % 2 else r for x, r in enumerate(reads)]
        groups.append((reads, [p, variant], [max(10, m // 16)] * 2))
    return _case(groups)


def _carry_chains():
    """all-A consensuses (every addition of the column carries through the whole word) and a short tandem repeat, against all-A, all-C and half-A reads"""
    reads = ["A" * 150, "C" * 150, "A" * 75 + "C" * 75, "C" * 70 + "A" * 140, "AC" * 90, "ACG" * 70, "A" * 260]
    return _case([(reads, ["A" * 130, "A" * 200, "AC" * 100, "T" * 130], [129, 60, 40, 30])])


def _read_lengths():
    """one wave that mixes a read of length 0, short reads and one long read; lengths around the pattern's and around the first two multiples of the staging chunk;
    the match at the read's last base and at its first possible column"""
    rng = np.random.default_rng(103)
    m = 100
    p = rand(rng, m); q = rand(rng, 70)
    reads = ["", "A", p[0], p[:m - 1], p, p + "G", p[1:], "T" + p]
    for L in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1):
        reads += [rand(rng, L - m) + p, p + rand(rng, L - m), rand(rng, L)]      # the match ends at the last base / begins at the first
    reads += [rand(rng, 500) + noisy(rng, p, 0.08) + rand(rng, 37), ref.revcomp(q), noisy(rng, q, 0.1)]
    return _case([(reads, [p, q], [12, 9])])


def _bounds():
    """d == k_c is a hit and d == k_c + 1 is not, on the same read by changing max_ed; max_ed of 0; max_ed >= m, clamped to m - 1; different bounds within one group:
    the nearest consensus is out of its bound and the second is reported as best"""
    rng = np.random.default_rng(104)
    p = rand(rng, 80)
    five = rand(rng, 30) + substitute(p, [5, 20, 35, 50, 65]) + rand(rng, 30)      # five substitutions, far apart: d = 5
    exact = rand(rng, 10) + p + rand(rng, 10)
    far = rand(rng, 120)
    reads = [five, exact, far, ""]
    near = substitute(p, [10, 40, 70])                                  # three from p; a read of p is 3 from it
    other = substitute(p, [1, 9, 17, 25, 33, 41, 49, 57, 73, 79])
    return _case([(reads, [p], [5]), (reads, [p], [4]), (reads, [p], [0]), (reads, [p], [80]), (reads, [p], [1 << 30]),
                  ([exact, five], [near, other], [2, 20]), ([exact, five], [near, other], [3, 20]),
                  (["A", "C", "AC"], ["A"], [7])])                      # m = 1: k_c = 0


def _reduction():
    """one consensus (cons2 = ed2 = -1); identical consensuses (the smaller index, ed2 == ed); best on strand 1; a consensus equal to its own reverse complement; a
    forward / reverse tie"""
    rng = np.random.default_rng(105)
    p = rand(rng, 90); q = substitute(p, [7, 30, 31, 64, 80])
    half = rand(rng, 40); pal = half + ref.revcomp(half)
    reads = [rand(rng, 12) + p + rand(rng, 9), ref.revcomp(rand(rng, 12) + q + rand(rng, 9)), rand(rng, 5) + noisy(rng, p, 0.06) + rand(rng, 5),
             ref.revcomp(noisy(rng, p, 0.06)), rand(rng, 200), rand(rng, 8) + pal + rand(rng, 8), ref.revcomp(rand(rng, 8) + substitute(pal, [3]) + rand(rng, 8)),
             p + rand(rng, 11) + ref.revcomp(p), substitute(ref.revcomp(p), [4]) + rand(rng, 11) + substitute(p, [60])]
    return [_case([(reads, [p], [20]), (reads, [p, p], [20, 20]), (reads, [q, p, q, p], [20] * 4), (reads, [pal, p], [20, 20]), (reads, [ref.revcomp(p), pal, q], [20, 20, 20])], both)
            for both in (True, False)]


def _groups():
    """groups of 1, 63, 64, 65 and 130 reads (more than one workgroup in all), a group with no read between two others, a group with no consensus, and 1, 2 and 7
    consensuses of unequal lengths that fall into different instances"""
    rng = np.random.default_rng(106)
    seven = [rand(rng, m) for m in (50, 100, 200, 300, 600, 900, 1100)]
    a, b, c, d, e = rand(rng, 100), rand(rng, 70), rand(rng, 90), rand(rng, 150), rand(rng, 130)

    def reads_of(n, sources):
        out = []
        for x in range(n):
            s = sources[x % len(sources)]
            body = noisy(rng, s, 0.05) if x % 5 else rand(rng, 60)
            r = rand(rng, int(rng.integers(0, 30))) + body + rand(rng, int(rng.integers(0, 30)))
            out.append(ref.revcomp(r) if x % 3 == 1 else r)
        return out
    one = [rand(rng, 10) + noisy(rng, seven[4], 0.04) + rand(rng, 10)]
    return _case([(one, seven, [m // 8 for m in (50, 100, 200, 300, 600, 900, 1100)]), (reads_of(63, [a, b]), [a, b], [15, 10]), (reads_of(64, [c]), [c], [13]),
                  ([], [d], [5]), (reads_of(65, [d, a]), [d, a], [22, 15]), (reads_of(3, [a]), [], []), (reads_of(130, [e, c]), [e], [19])])


CUTOFF_PLANTED = None                                                   # set by _cutoff: the read numbers that hold a true match


def _cutoff():
    """the cases of the cut-off rule: 300 to 600 unrelated letters followed by the true match (blocks must re-enter after they fell idle); the match first and the
    unrelated letters after it; a wave where one lane matches fully and 63 do not"""
    global CUTOFF_PLANTED
    rng = np.random.default_rng(107)
    p, q = rand(rng, 300), rand(rng, 280)
    late = [rand(rng, int(rng.integers(300, 601))) + noisy(rng, (p, q)[x % 2], 0.05) for x in range(24)]
    early = [noisy(rng, (p, q)[x % 2], 0.05) + rand(rng, int(rng.integers(300, 601))) for x in range(24)]
    lone = [rand(rng, 350) for _ in range(64)]; lone[37] = rand(rng, 40) + p + rand(rng, 10)
    late = [ref.revcomp(r) if x % 4 == 3 else r for x, r in enumerate(late)]
    CUTOFF_PLANTED = list(range(48)) + [48 + 37]
    return _case([(late, [p, q], [45, 42]), (early, [p, q], [45, 42]), (lone, [p, q], [45, 42])])


_BUILDERS = {"pattern_lengths": _pattern_lengths, "carry_chains": _carry_chains, "read_lengths": _read_lengths, "bounds": _bounds,
             "reduction_both": lambda: _reduction()[0], "reduction_one_strand": lambda: _reduction()[1], "groups": _groups, "cutoff": _cutoff}
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def build(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    c = build(name)
    hits = ref.recruit(c["reads"], c["read_off"], c["cons"], c["cons_off"], c["max_ed"], c["both"])
    hits.setflags(write=False)
    return hits


def pair_strands(name):
    """every (pattern strand, read, k_c) of a case, identical triples once"""
    c = build(name)
    seen = set()
    for g in range(len(c["read_off"]) - 1):
        for ci in range(int(c["cons_off"][g]), int(c["cons_off"][g + 1])):
            for p in (c["cons"][ci], ref.revcomp(c["cons"][ci])):
                for r in range(int(c["read_off"][g]), int(c["read_off"][g + 1])):
                    t = (p, c["reads"][r], min(int(c["max_ed"][ci]), len(p) - 1))
                    if t not in seen:
                        seen.add(t); yield t
