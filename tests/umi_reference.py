"""Independent restatement of include/ngsid_umi.h and of the policy of ngspeciesid_amd/umi.py in plain loops - test infrastructure, not a test.  Pairs by
variants_reference's edit distance over all i < j, centroids by variants_reference.cluster, extraction through demux_reference.locate.  Shares no code with either."""
import numpy as np
import variants_reference as vr
import demux_reference as dr


def pairs(seqs, max_dist):
    """brute force over all i < j -> [(i, j, dist)] in ascending (i, j) order"""
    out = []
    for i in range(len(seqs) - 1):
        f = vr.ed_many(seqs[i], list(seqs[i + 1:]))
        out += [(i, i + 1 + k, int(f[k])) for k in range(len(f)) if f[k] <= max_dist]
    return out


def centroids(pair_list, order, n):
    """the nodes walked in `order`, each joining the earliest-founded centroid it has a listed pair with -> (bin_of [n], centroid [n_bins]): variants_reference.cluster
    with a constant threshold and sizes that spell the order out"""
    rank = {x: k for k, x in enumerate(order)}
    sizes = [n - rank[x] for x in range(n)]
    bin_of, cents, _, _ = vr.cluster(sizes, [0] * n, [""] * n, [(i, j, 0, 0) for i, j, *_ in pair_list], lambda i, j: 0)
    return bin_of, cents


def extract(reads, flanks, umi_len, len_slack, window, flank_max_ed, lib=None, prefix="ngsid_"):
    """flanks = (fwd_pre, fwd_post, rev_pre, rev_post) -> per read (status, strand, key, cut0, cut1): status 'ok' / 'no_umi' / 'bad_len', strand '+' / '-' / None"""
    H = [dr.locate(reads, [f], window, flank_max_ed, True, lib=lib, prefix=prefix)[0] for f in flanks]
    out = []
    for r, read in enumerate(reads):
        wins = dr.side_windows(read, window)
        def pair(pre, post, side):
            a, b = H[pre][r, side], H[post][r, side]
            if a[0] < 0 or b[0] < 0 or not a[3] < b[2]: return None
            return dict(u=wins[side][int(a[3]) + 1:int(b[2])].decode(), ed=int(a[1]) + int(b[1]), cut=int(b[3]) + 1)
        cands, placed = [], False
        for name, (fs, rs_) in (("+", (0, 1)), ("-", (1, 0))):
            f, v = pair(0, 1, fs), pair(2, 3, rs_)
            if f is None or v is None: continue
            placed = True
            if abs(len(f["u"]) - umi_len) <= len_slack and abs(len(v["u"]) - umi_len) <= len_slack:
                cuts = (f["cut"], v["cut"]) if name == "+" else (v["cut"], f["cut"])
                cands.append((f["ed"] + v["ed"], name, f["u"] + v["u"], cuts))
        if cands:
            best = min(cands, key=lambda c: (c[0], c[1] != "+"))
            out.append(("ok", best[1], best[2], best[3][0], best[3][1]))
        else:
            out.append(("bad_len" if placed else "no_umi", None, None, 0, 0))
    return out


def bins(keys, max_dist, min_reads):
    """keys per read (None: no key) -> (bin of every read or -1, [(centroid key, reads, distinct)] per bin in founding order, small [B])"""
    umis = sorted({k for k in keys if k is not None})
    counts = [sum(1 for k in keys if k == u) for u in umis]
    order = sorted(range(len(umis)), key=lambda x: (-counts[x], -len(umis[x]), umis[x].encode(), x))
    bin_of, cents = centroids(pairs(umis, max_dist), order, len(umis))
    at = {u: i for i, u in enumerate(umis)}
    rbin = [bin_of[at[k]] if k is not None else -1 for k in keys]
    rows = [(umis[c], sum(counts[x] for x in range(len(umis)) if bin_of[x] == b), sum(1 for x in range(len(umis)) if bin_of[x] == b)) for b, c in enumerate(cents)]
    return rbin, rows, [row[1] < min_reads for row in rows]
