"""Settles the thresholds of ngspeciesid_amd/hp.py (the homopolymer run-length vote) on the CPU, with the reference definition of the device call (tests/hp_reference.py on
the oracle) - no GPU.

Sets: C3's read profile (5 species of 750 bases at 15 % divergence, mu = 17, k = 13, w = 20, three polishing iterations), 400 reads a set dealt 5 / 10 / 20 / 25 / 40 %
to the species, so the clusters hold from about 20 to about 160 reads; every template also gets six planted runs of 5 - 7 bases.
Read model, ON TOP of synth.make_reads and MADE UP (no data behind the rates - it only has the shape of the error the plain model lacks): after the ordinary errors every
run of a read of at least 3 bases is shortened by one with probability min(0.9, L * rate * f), else lengthened by one with probability L * rate * f / 4, where L is the run's
length and f = 1 on the plus strand and 0.6 on the minus strand.  rate = 0: the plain model.
Condition (a), no harm: over the unbiased sets, the consensuses that already equal their amplicon - the pass changes no base.
Condition (b), improvement: the rate is raised until the pipeline WITHOUT the pass leaves a wrong run length in at least a quarter of the consensuses; on those sets the
pass leaves no set with more wrong runs than before, and fewer in total.
A consensus is compared with its amplicon run by run: its run letters must be a contiguous part of the amplicon's (either strand; the ends may be trimmed), the first and
the last run of the consensus are not compared; a consensus with another kind of error is counted as `unmatched` and left out of the run counts.
Every grid row runs the full pass (hp.polish, both rounds).  Usage: python tools/hp_sweep.py [--seeds 20] [--jobs 8] > profiles/hp.txt (the tool prints the section of
the sweep; tools/hp_bench.py appends the timings)"""
import argparse, itertools, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

ABUNDANCE = (0.05, 0.10, 0.20, 0.25, 0.40)
GRID = dict(min_depth=(6, 8, 12), min_share=(0.4, 0.5, 0.6), min_margin=(0.1, 0.2, 0.3), min_strand_depth=(4, 10 ** 9))
SIZE_BINS = ((0, 30), (30, 60), (60, 120), (120, 10 ** 9))


def _runs(s):
    from ngspeciesid_amd import hp
    st, ln = hp.runs(s)
    return "".join(s[int(a)] for a in st), ln


def templates(seed):
    from ngspeciesid_amd import synth
    rng = np.random.default_rng(1000 + seed); out = []
    for s in synth.make_species(5, 750, 0.15, seed=seed):
        t = list(s.tobytes().decode())
        for i in range(6):
            p = 60 + 110 * i + int(rng.integers(20)); letter = "ACGT"[int(rng.integers(4))]
            t[p:p + 5 + i % 3] = letter * (5 + i % 3)
        out.append("".join(t))
    return out


def biased_reads(T, n, seed, rate):
    """synth.make_reads, then the made-up length bias of the module text -> a host ReadSet with qualities"""
    from ngspeciesid_amd import synth
    from ngspeciesid_amd._capi import ReadSet
    rd = synth.make_reads([np.frombuffer(t.encode(), dtype=np.uint8).copy() for t in T], n, mu=17.0, seed=seed, abundance=list(ABUNDANCE), rc_fraction=0.5)
    seq, qual, off, strand = rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy(), rd["strand"].numpy()
    if rate <= 0: return ReadSet(seq, qual, off.astype(np.uint64))
    rng = np.random.default_rng(seed + 77); seqs, quals = [], []
    for i in range(len(off) - 1):
        s = seq[off[i]:off[i + 1]]; q = qual[off[i]:off[i + 1]]; f = 0.6 if strand[i] else 1.0
        b = np.concatenate(([0], np.nonzero(s[1:] != s[:-1])[0] + 1, [len(s)])); rep = np.ones(len(s), dtype=np.int64)
        for x, y in zip(b[:-1], b[1:]):
            L = int(y - x)
            if L < 3: continue
            u = rng.random()
            if u < min(0.9, L * rate * f): rep[x] = 0
            elif u < min(0.9, L * rate * f) + L * rate * f / 4: rep[x] = 2
        seqs.append(np.repeat(s, rep)); quals.append(np.repeat(q, rep))
    o = np.zeros(len(seqs) + 1, dtype=np.uint64); o[1:] = np.cumsum([len(x) for x in seqs])
    return ReadSet(np.concatenate(seqs), np.concatenate(quals), o)


def compare(cons, T):
    """-> (template, its run lengths over the consensus's runs, consensus run lengths) with the first and last run cut, or None (unmatched)"""
    from ngspeciesid_amd.pipeline import revcomp_str
    cl, cn = _runs(cons)
    for t in T:
        for tt in (t, revcomp_str(t)):
            tl, tn = _runs(tt)
            at = tl.find(cl)
            if at >= 0 and len(cl) >= 3: return tt, tn[at + 1:at + len(cl) - 1], cn[1:-1]
    return None


class _Cached:
    """the reference adapter with the histogram calls remembered: every grid row asks the same first round"""
    def __init__(self, api):
        self._api, self._memo = api, {}

    def __getattr__(self, name):
        return getattr(self._api, name)

    def hp_runs(self, centres, rs, grp_off, run_off, run_start, read_order=None, k=13, w=20, clip=False):
        key = (tuple(centres.get(i)[0] for i in range(centres.n)), np.asarray(read_order).tobytes(), np.asarray(run_start).tobytes())
        if key not in self._memo: self._memo[key] = self._api.hp_runs(centres, rs, grp_off, run_off, run_start, read_order=read_order, k=k, w=w, clip=clip)
        return self._memo[key]


def one_set(job):
    """one read set through the pipeline without the pass, then the pass under every grid row -> per consensus (size, equal, unmatched, true and own run lengths,
    per row: run lengths after, bases changed)"""
    seed, rate, rows = job
    from oracle_lib import load_oracle
    from hp_reference import HpAdapter
    from ngspeciesid_amd import pipeline, hp
    from ngspeciesid_amd.hostutil import subset_reads
    from ngspeciesid_amd.ptable import select_p_table
    from ngspeciesid_amd.pipeline import revcomp_str
    orc = load_oracle(); api = _Cached(HpAdapter(orc))
    T = templates(seed); rs = biased_reads(T, 400, 50 + seed, rate)
    score, err, keep = orc.score_reads(rs, 13, 7.0)
    idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
    sub = subset_reads(rs, idx)
    res = pipeline.run_hot_path(orc, sub, score[idx], acc_rank=np.arange(sub.n, dtype=np.uint32), k=13, w=20, abundance_ratio=0.02, racon_iter=3, band=0, p_shared=select_p_table(13, 20))
    seqs = [c[3] for c in res["centers"]]
    lists = [np.concatenate([np.nonzero(res["rep_of"] == r)[0] for r in c[4]]).astype(np.uint32) for c in res["centers"]]
    after = [hp.polish(api, seqs, sub, lists, k=13, w=20, rounds=2, **row)[0] for row in rows]
    out = []
    for i, q in enumerate(seqs):
        cmp0 = compare(q, T)
        equal = any(q in t or q in revcomp_str(t) for t in T)
        rec = dict(size=len(lists[i]), equal=equal, unmatched=cmp0 is None, true=None if cmp0 is None else cmp0[1], own=None if cmp0 is None else cmp0[2], rows=[])
        for a in after:
            cmp1 = compare(a[i], T)
            rec["rows"].append((None if cmp1 is None else cmp1[2], sum(1 for x, y in zip(_runs(q)[1], _runs(a[i])[1]) if x != y)))
        out.append(rec)
    return seed, rate, out


def summarise(results, r):
    """grid row r over the sets of one rate -> (consensuses, with a wrong run before, wrong runs before, after, sets worse, runs changed in the equal consensuses, equal ones)"""
    n = bad = wb = wa = worse = harm = eq = 0
    for _, _, recs in results:
        sb = sa = 0
        for c in recs:
            if c["equal"]: eq += 1; harm += c["rows"][r][1]
            if c["unmatched"] or c["rows"][r][0] is None: continue
            n += 1; b = int((c["own"] != c["true"]).sum()); a = int((c["rows"][r][0] != c["true"]).sum())
            bad += b > 0; sb += b; sa += a
        wb += sb; wa += sa; worse += sa > sb
    return n, bad, wb, wa, worse, harm, eq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--rates", type=float, nargs="*", default=[0.02, 0.03, 0.04, 0.05, 0.06])
    a = ap.parse_args()
    from multiprocessing import Pool
    from ngspeciesid_amd import hp
    keys = sorted(GRID); rows = [dict(zip(keys, v)) for v in itertools.product(*(GRID[k] for k in keys))]
    if hp.DEFAULTS not in rows: rows.append(dict(hp.DEFAULTS))
    dflt = rows.index(dict(hp.DEFAULTS))
    print("# homopolymer run-length vote: threshold sweep on the CPU reference (tools/hp_sweep.py).  The read model's length bias is MADE UP (see the tool's text).")
    print("# %d seeds x 5 clusters, 400 reads a set, clusters of about 20 - 160 reads; grid %s; shipped defaults %s" % (a.seeds, GRID, hp.DEFAULTS))
    with Pool(a.jobs) as pool:
        plain = pool.map(one_set, [(s, 0.0, rows) for s in range(a.seeds)])
        biased, rate = None, None
        for rate in a.rates:
            biased = pool.map(one_set, [(s, rate, rows) for s in range(a.seeds)])
            n, bad = summarise(biased, dflt)[:2]
            print("# rate %.2f without the pass: %d of %d consensuses carry a wrong run length" % (rate, bad, n))
            if 4 * bad >= n: break
    print("# condition (b) is judged at rate %.2f; condition (a) on the unbiased sets" % rate)
    print("# row: thresholds | (a) runs changed in the consensuses equal to their amplicon (of how many such) | (b) wrong runs before -> after, sets worse | meets both")
    ok_rows = []
    for r, row in enumerate(rows):
        _, _, _, _, _, harm, eq = summarise(plain, r)
        n, bad, wb, wa, worse, _, _ = summarise(biased, r)
        ok = harm == 0 and worse == 0 and wa < wb
        if ok: ok_rows.append((wa, r))
        print("%s | %d (%d) | %d -> %d, %d | %s%s" % (" ".join("%s=%s" % (k, "off" if row[k] >= 10 ** 9 else row[k]) for k in keys), harm, eq, wb, wa, worse, "yes" if ok else "no", "   <- shipped" if r == dflt else ""))
    print("# rows that meet both: %d of %d; fewest wrong runs left among them: %s" % (len(ok_rows), len(rows), " ".join("%s=%s" % (k, rows[min(ok_rows)[1]][k]) for k in keys) if ok_rows else "none"))
    print("# shipped defaults on the unbiased sets too: wrong runs %d -> %d" % summarise(plain, dflt)[2:4])
    print("# recall of the shipped defaults at rate %.2f (wrong runs of the consensus before the pass: repaired / all), and runs that were right and are wrong after" % rate)
    by_len, by_size, broke = {}, {}, 0
    for _, _, recs in biased:
        for c in recs:
            if c["unmatched"] or c["rows"][dflt][0] is None: continue
            aft = c["rows"][dflt][0]; b = next(i for i, (lo, hi) in enumerate(SIZE_BINS) if lo <= c["size"] < hi)
            for t, o, x in zip(c["true"], c["own"], aft):
                if o != t:
                    for d, key in ((by_len, int(t)), (by_size, b)):
                        d.setdefault(key, [0, 0]); d[key][1] += 1; d[key][0] += int(x == t)
                elif x != t: broke += 1
    print("by true run length: " + "  ".join("%d: %d/%d" % (k, v[0], v[1]) for k, v in sorted(by_len.items())))
    print("by cluster size: " + "  ".join("%s: %d/%d" % ("%d-%d" % SIZE_BINS[k] if SIZE_BINS[k][1] < 10 ** 9 else "%d+" % SIZE_BINS[k][0], v[0], v[1]) for k, v in sorted(by_size.items())))
    print("right before, wrong after: %d" % broke)
    print("unmatched consensuses (another kind of error; left out): unbiased %d, biased %d" % (sum(c["unmatched"] for _, _, r in plain for c in r), sum(c["unmatched"] for _, _, r in biased for c in r)))


if __name__ == "__main__":
    main()
