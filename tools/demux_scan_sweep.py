#!/usr/bin/env python3
"""Settles the default of --demux_mid_max_ed (ngspeciesid_amd/demux.py default_mid_max_ed) on the CPU reference (tests/demux_scan_reference.py); no GPU.

Per tag length (13, 16 and 24 bases): a dual-tag pool of 4 samples (tests/demux_reference.py make_pool: noisy amplicon reads of about 320 bases, every tag with 0-3
planted edits, 0-30 random bases outside the tags, a share of the reads reverse-complemented) and the two-amplicon concatemers of consecutive read pairs.  Every read
goes through the policy as the command line runs it: the end tags by the locator's definition (window 150, max_ed 3) and assign(), the whole read by the scan's
definition at the bound under test, interior_hits().  Per bound: the clean reads with an interior hit (must be none), the concatemers with at least one (recall), and
the concatemers with exactly their two junction hits.

The rule: per tag length the bounds at which no clean read has an interior hit are eligible; among them the one with the highest recall, the smallest on a tie.

    python tools/demux_scan_sweep.py [--reads 100] >> profiles/demux.txt
"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import demux_reference as ref
import demux_scan_reference as sref
from ngspeciesid_amd import demux

BOUNDS = (0, 1, 2, 3, 4)
TAG_SETS = ((13, 5), (16, 6), (24, 9))          # tag length, smallest edit distance between any two tags (and reverse complements)


def interior_counts(reads, sheet, patterns, plen):
    """-> counts [len(BOUNDS)][n]: interior hits of every read at every bound"""
    lens = np.array([len(r) for r in reads])
    hits = ref.locate(reads, sheet.tags, 150, 3, True)[0]
    result = demux.assign(hits, sheet, 2, lens=lens)
    rows = [[sref.last_row(p, r, True) for p in patterns] for r in reads]          # the scores do not depend on the bound
    out = np.zeros((len(BOUNDS), len(reads)), dtype=np.int64)
    for b, bound in enumerate(BOUNDS):
        hit_off = np.zeros(len(reads) + 1, dtype=np.int64); recs = []
        for r in range(len(reads)):
            recs += [(p, e, d) for p in range(len(patterns)) for e, d in sref.runs_to_hits(rows[r][p], min(bound, plen[p] - 1))]
            hit_off[r + 1] = len(recs)
        inner = demux.interior_hits(hit_off, np.array(recs, dtype=np.int64).reshape(-1, 3), plen, lens, result[3], result[4], bound)
        out[b] = np.bincount(np.repeat(np.arange(len(reads)), np.diff(hit_off))[inner], minlength=len(reads))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100, help="clean reads per sample (4 samples); half as many concatemers per sample")
    args = ap.parse_args()
    print("# tools/demux_scan_sweep.py --reads %d: interior hits by the numpy reference; clean = reads of one amplicon, conc = two amplicons joined end to end" % args.reads)
    print("# tag_len\tbound\tclean_reads\tclean_with_interior_hit\tconcatemers\tconc_detected\tconc_with_exactly_2_hits\trecall")
    chosen = {}
    for m, min_dist in TAG_SETS:
        t0 = time.time()
        tags = ref.make_tags(8, m, min_dist, seed=5)
        fwd, rev = tags[0::2], tags[1::2]
        sheet = demux.Sheet(["s%d" % s for s in range(4)], tags, [0, 2, 4, 6], [1, 3, 5, 7])
        patterns = demux.scan_patterns(sheet); plen = np.array([len(p) for p in patterns])
        pool = ref.make_pool(fwd, rev, args.reads, seed=3, junk_reads=0, max_edits=3)
        clean = pool["seqs"]
        conc = sref.make_concatemers(pool, [(2 * i, 2 * i + 1) for i in range(len(clean) // 2)])[0]
        c_clean = interior_counts(clean, sheet, patterns, plen); c_conc = interior_counts(conc, sheet, patterns, plen)
        best = None
        for b, bound in enumerate(BOUNDS):
            fp = int((c_clean[b] > 0).sum()); det = int((c_conc[b] > 0).sum()); two = int((c_conc[b] == 2).sum())
            print("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.3f" % (m, bound, len(clean), fp, len(conc), det, two, det / len(conc)))
            if fp == 0 and (best is None or det > best[1]):
                best = (bound, det)
        chosen[m] = best[0] if best else None
        print("# tag_len %d: chosen bound %s, default_mid_max_ed(%d) = %d (%.0f s)" % (m, chosen[m], m, demux.default_mid_max_ed(m), time.time() - t0), flush=True)
    print("# rule: " + ", ".join("%d bases -> %s" % (m, b) for m, b in chosen.items()))


if __name__ == "__main__":
    main()
