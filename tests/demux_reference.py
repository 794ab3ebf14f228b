"""The definition of ngsid_demux_locate (include/ngsid_demux.h), restated slowly - test infrastructure, not a test.

Windows and reverse complements are built in numpy, every (window, tag) pair goes through the host locator (ngsid_host_infix_locate, or the oracle's twin with
lib=oracle.lib, prefix="ongsid_"), the reduction per (read, side) is done in numpy.  Also the generator of pooled reads with known truth."""
import ctypes as C
import numpy as np
from ngspeciesid_amd import synth

_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    _COMP[_a] = _b


def revcomp(s: str) -> str:
    return _COMP[np.frombuffer(s.encode(), dtype=np.uint8)[::-1]].tobytes().decode()


def side_windows(read: str, window: int):
    """(side 0 window, side 1 window): read[0 : min(W, L)] and the first min(W, L) bases of the reverse complement"""
    a = np.frombuffer(read.encode(), dtype=np.uint8)
    w = min(window, len(a))
    return a[:w].tobytes(), _COMP[a[::-1][:w]].tobytes()


def locate(reads, tags, window, max_ed, iupac=True, lib=None, prefix="ngsid_"):
    """-> (hits [n, 2, 5] int32, ed_all [n, 2, T] int16, end_all [n, 2, T] int16)"""
    if lib is None:
        from ngspeciesid_amd import runtime
        lib = runtime.load_library()
    fn = getattr(lib, prefix + "host_infix_locate")
    n, T = len(reads), len(tags)
    tg = [t.encode() for t in tags]
    ed_all = np.full((n, 2, T), -1, dtype=np.int16); end_all = np.full((n, 2, T), -1, dtype=np.int16); start_all = np.full((n, 2, T), -1, dtype=np.int32)
    ed, st, en = C.c_int32(), C.c_int32(), C.c_int32()
    for r, read in enumerate(reads):
        for side, win in enumerate(side_windows(read, window)):
            for t, q in enumerate(tg):
                rc = fn(q, C.c_int32(len(q)), win, C.c_int32(len(win)), C.c_int32(int(max_ed)), C.c_int32(int(iupac)), C.byref(ed), C.byref(st), C.byref(en))
                assert rc == 0
                ed_all[r, side, t], end_all[r, side, t], start_all[r, side, t] = ed.value, en.value, st.value
    hits = np.full((n, 2, 5), -1, dtype=np.int32)
    if n and T:
        big = np.where(ed_all >= 0, ed_all.astype(np.int32), 1 << 20)
        best = big.argmin(axis=2)                                      # the smallest ed; on equal ed the smallest index
        bed = np.take_along_axis(big, best[:, :, None], 2)[:, :, 0]
        has = bed < (1 << 20)
        other = big.copy(); np.put_along_axis(other, best[:, :, None], 1 << 20, 2)
        ed2 = other.min(axis=2)
        hits[:, :, 0] = np.where(has, best, -1)
        hits[:, :, 1] = np.where(has, bed, -1)
        hits[:, :, 2] = np.where(has, np.take_along_axis(start_all, best[:, :, None], 2)[:, :, 0], -1)
        hits[:, :, 3] = np.where(has, np.take_along_axis(end_all.astype(np.int32), best[:, :, None], 2)[:, :, 0], -1)
        hits[:, :, 4] = np.where(has & (ed2 < (1 << 20)), ed2, -1)
    return hits, ed_all, end_all


def edit_distance(a: str, b: str) -> int:
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[-1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def make_tags(n, length=24, min_dist=9, seed=5):
    """n random ACGT tags drawn by rejection: any two, and any one against another's reverse complement, are at least min_dist edits apart"""
    rng = np.random.default_rng(seed)
    tags = []
    while len(tags) < n:
        t = "".join("ACGT"[i] for i in rng.integers(0, 4, length))
        if all(edit_distance(t, u) >= min_dist and edit_distance(t, revcomp(u)) >= min_dist for u in tags) and edit_distance(t, revcomp(t)) >= min_dist:
            tags.append(t)
    return tags


def _edit(tag, k, rng):
    s = list(tag)
    for _ in range(k):
        kind = rng.integers(0, 3); p = int(rng.integers(0, len(s)))
        if kind == 0: s[p] = "ACGT"[("ACGT".index(s[p]) + int(rng.integers(1, 4))) % 4]
        elif kind == 1: s.insert(p, "ACGT"[int(rng.integers(0, 4))])
        elif len(s) > 1: del s[p]
    return "".join(s)


def _junk(k, rng):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, k))


def make_pool(fwd, rev, reads_per_sample, seed, n_species=2, length=320, junk_reads=10, mu=20.0, rc_fraction=0.3, max_edits=4, samples=None):
    """Pooled reads: per sample s (of `samples`, default all) reads_per_sample noisy amplicon reads (synth), each as
    junk(0..30) + edited fwd[s] + amplicon + reverse complement of the edited rev[s] + junk(0..30), a share of them reverse-complemented as a whole;
    + junk_reads reads per sample whose forward tag is replaced by random bases.  Shuffled.
    -> dict(seqs, quals, names, sample, strand, edits [n, 2] (planted edits of the forward and the reverse tag), junk [n] bool)"""
    rng = np.random.default_rng(seed)
    samples = list(range(len(fwd))) if samples is None else list(samples)
    sp = synth.make_species(n_species, length, 0.15, seed=seed + 1)
    rows = []
    for s in samples:
        rd = synth.make_reads(sp, reads_per_sample + junk_reads, mu=mu, seed=seed * 100 + s)
        seq, qual, off = rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy()
        for i in range(reads_per_sample + junk_reads):
            a = seq[off[i]:off[i + 1]].tobytes().decode(); q = qual[off[i]:off[i + 1]].tobytes().decode()
            junk = i >= reads_per_sample
            ef, er = int(rng.integers(0, max_edits + 1)), int(rng.integers(0, max_edits + 1))
            head = _junk(int(rng.integers(0, 31)), rng) + (_junk(len(fwd[s]), rng) if junk else _edit(fwd[s], ef, rng))
            tail = revcomp(_edit(rev[s], er, rng)) + _junk(int(rng.integers(0, 31)), rng)
            read = head + a + tail; rq = "I" * len(head) + q + "I" * len(tail)
            strand = int(rng.random() < rc_fraction)
            if strand: read, rq = revcomp(read), rq[::-1]
            rows.append((read, rq, s, strand, ef, er, junk))
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    return dict(seqs=[r[0] for r in rows], quals=[r[1] for r in rows], names=["read%d s%d" % (i, r[2]) for i, r in enumerate(rows)],
                sample=np.array([r[2] for r in rows]), strand=np.array([r[3] for r in rows]), edits=np.array([[r[4], r[5]] for r in rows]).reshape(-1, 2),
                junk=np.array([r[6] for r in rows], dtype=bool))


def write_fastq(path, names, seqs, quals):
    with open(path, "w") as f:
        for nm, s, q in zip(names, seqs, quals):
            f.write("@%s\n%s\n+\n%s\n" % (nm, s, q))
