"""The study-wide variant table of a multi-sample run (extension; `--variants`, sub-command `variants`): the policy on top of ngsid_near_pairs and, with
`--variant_wide_max_dist`, ngsid_near_pairs_wide (include/ngsid_near.h, csrc/k_near.hip).

The library returns, for the final consensuses of all samples together, every pair that lies within a few edits on either strand, as integers.  What a variant is -
the admissible distance of a pair, which sequence stands for its neighbours, the tables - is decided here, in Python and numpy, and no device call is made except
through `api`.

The rule is the one amplicon users know as cluster-by-size: the sequences are walked by abundance, a sequence joins the earliest centroid within its pair threshold
and founds a variant otherwise.  Classifying the variants, calling index hops and cross-sample chimeras are not done here; variant_members.tsv is what they start from.
"""
from __future__ import annotations
import os
import numpy as np
from . import classify
from ._capi import ReadSet, NEAR_MAX_DIST, NEAR_WIDE_MAX_DIST

DEFAULTS = dict(identity="0.97", max_dist=NEAR_MAX_DIST, wide_max_dist=None)
MEMBER_COLUMNS = ("sample", "consensus id", "reads", "variant", "dist", "strand")
_TEXT = ("sample", "consensus id", "variant", "strand")


def collect(groups):
    """groups = [(sample name, folder, [(consensus id, n_reads, sequence)])], what the chimera step receives -> dict(samples [S] names, seqs [n], sizes [n] int64,
    sample [n] int64 = index into samples, ids [n]): every final consensus of every group, in group order"""
    samples = [g[0] for g in groups]
    seqs = [s for _, _, cons in groups for _, _, s in cons]
    return dict(samples=samples, seqs=seqs, ids=[c for _, _, cons in groups for c, _, _ in cons],
                sizes=np.array([nr for _, _, cons in groups for _, nr, _ in cons], dtype=np.int64),
                sample=np.array([x for x, (_, _, cons) in enumerate(groups) for _ in cons], dtype=np.int64))


def _identity_fraction(identity):
    """a decimal string such as '0.97' -> (numerator, denominator) integers, no float in between"""
    text = str(identity).strip()
    whole, dot, frac = text.partition(".")
    if not (whole + frac).isdigit() or (dot and not frac):
        raise ValueError("--variant_identity must be a decimal fraction such as 0.97, not %r" % (identity,))
    num, den = int(whole + frac), 10 ** len(frac)
    if not 0 <= num <= den:
        raise ValueError("--variant_identity is a fraction in [0, 1], not %r" % (identity,))
    return num, den


def thresholds(lengths, identity, max_dist, wide_max_dist=None):
    """the admissible distance of every pair: thr(i, j) = min(max_dist, floor((1 - identity) * max(len_i, len_j))).  identity is a decimal STRING ('0.97'); the
    product is formed once, in integer arithmetic, as ((den - num) * length) // den with identity = num / den, so that 0.97 of 600 bases is exactly 18 edits and never
    17 by a float's last bit.  Since the bound grows with the length, thr(i, j) is the larger of the two per-sequence values
    -> (t int64 [n] with thr(i, j) = max(t[i], t[j]), K = the largest of them = the max_dist the device call is made with).  A max_dist above NEAR_MAX_DIST is a
    ValueError that names the flag: the one-word band of the kernel holds 31 edits, and a silently smaller bound would split variants the user asked to join.
    wide_max_dist (--variant_wide_max_dist, 0 .. NEAR_WIDE_MAX_DIST), when given, replaces max_dist as the edit bound (max_dist is then not looked at): the call
    goes to the wide kernels."""
    if wide_max_dist is not None:
        max_dist = int(wide_max_dist)
        if not 0 <= max_dist <= NEAR_WIDE_MAX_DIST:
            raise ValueError("--variant_wide_max_dist must be 0..%d (the widest device band holds %d edits), not %d" % (NEAR_WIDE_MAX_DIST, NEAR_WIDE_MAX_DIST, max_dist))
    else:
        max_dist = int(max_dist)
        if not 0 <= max_dist <= NEAR_MAX_DIST:
            raise ValueError("--variant_max_dist must be 0..%d (the one-word device band holds %d edits; --variant_wide_max_dist goes up to %d), not %d"
                             % (NEAR_MAX_DIST, NEAR_MAX_DIST, NEAR_WIDE_MAX_DIST, max_dist))
    num, den = _identity_fraction(identity)
    t = np.array([min(max_dist, ((den - num) * int(L)) // den) for L in lengths], dtype=np.int64)
    return t, (int(t.max()) if len(t) else 0)


def cluster(sizes, lengths, seqs, pairs, dist, thr, strand=None):
    """greedy abundance-ordered centroid clustering.  pairs = (pair_i, pair_j) and dist (strand) as Api.near_pairs returns them, thr = the per-sequence array of
    thresholds().  The sequences are ordered by reads descending, length descending, sequence bytes ascending, index ascending and walked in that order: a sequence
    joins the earliest-founded centroid it has a pair with at dist <= max(thr[i], thr[j]), else it founds a variant.  Deterministic, and independent of the order
    of the input -> (variant_of int64 [n], centroids [V] sequence indices in founding order, member_dist int64 [n], member_strand int64 [n]; 0 / 0 for a centroid)"""
    n = len(seqs)
    pi, pj = np.asarray(pairs[0], dtype=np.int64), np.asarray(pairs[1], dtype=np.int64)
    dist = np.asarray(dist, dtype=np.int64); strand = np.zeros(len(dist), dtype=np.int64) if strand is None else np.asarray(strand, dtype=np.int64)
    thr = np.asarray(thr, dtype=np.int64)
    nb = [[] for _ in range(n)]
    for a, b, d, s in zip(pi.tolist(), pj.tolist(), dist.tolist(), strand.tolist()):
        if d <= max(int(thr[a]), int(thr[b])):
            nb[a].append((b, d, s)); nb[b].append((a, d, s))
    order = sorted(range(n), key=lambda x: (-int(sizes[x]), -int(lengths[x]), seqs[x].encode(), x))
    variant_of = np.full(n, -1, dtype=np.int64); mdist = np.zeros(n, dtype=np.int64); mstrand = np.zeros(n, dtype=np.int64)
    centroids, is_centroid = [], np.zeros(n, dtype=bool)
    for x in order:
        best = None
        for y, d, s in nb[x]:
            if is_centroid[y] and (best is None or variant_of[y] < best[0]): best = (int(variant_of[y]), d, s)
        if best is None:
            variant_of[x] = len(centroids); centroids.append(x); is_centroid[x] = True
        else:
            variant_of[x], mdist[x], mstrand[x] = best
    return variant_of, centroids, mdist, mstrand


def table(col, variant_of, centroids, mdist, mstrand):
    """col = collect(...) and the result of cluster() -> dict(samples, variants = [dict(name, seq, size, n_samples)], counts int64 [V, S] read counts,
    members = [dict over MEMBER_COLUMNS] in input order)"""
    S, V = len(col["samples"]), len(centroids)
    if any(str(s) == "variant" for s in col["samples"]): raise ValueError("a sample cannot be called 'variant': it is a column of variant_table.tsv")
    counts = np.zeros((V, S), dtype=np.int64)
    np.add.at(counts, (np.asarray(variant_of, dtype=np.int64), col["sample"]), col["sizes"])
    names = ["variant_%d" % v for v in range(V)]
    variants = [dict(name=names[v], seq=col["seqs"][c], size=int(counts[v].sum()), n_samples=int((counts[v] > 0).sum())) for v, c in enumerate(centroids)]
    members = [dict(zip(MEMBER_COLUMNS, (col["samples"][int(col["sample"][x])], col["ids"][x], int(col["sizes"][x]), names[int(variant_of[x])], int(mdist[x]), "+-"[int(mstrand[x])])))
               for x in range(len(col["seqs"]))]
    return dict(samples=list(col["samples"]), variants=variants, counts=counts, members=members)


def write(outfolder, tab):
    """variants.fasta (the centroid sequences as they are, `>variant_{v};size={reads};samples={n}`), variant_table.tsv (one row per variant, one column per sample,
    read counts), variant_members.tsv (MEMBER_COLUMNS); tab-separated, one header line starting with '#', like the other tables"""
    with open(os.path.join(outfolder, "variants.fasta"), "w") as fh:
        for v in tab["variants"]:
            fh.write(">%s;size=%d;samples=%d\n%s\n" % (v["name"], v["size"], v["n_samples"], v["seq"]))
    with open(os.path.join(outfolder, "variant_table.tsv"), "w") as fh:
        fh.write("#" + "\t".join(["variant"] + [str(s) for s in tab["samples"]]) + "\n")
        for v, row in zip(tab["variants"], tab["counts"]):
            fh.write("\t".join([v["name"]] + [str(int(x)) for x in row]) + "\n")
    with open(os.path.join(outfolder, "variant_members.tsv"), "w") as fh:
        fh.write("#" + "\t".join(MEMBER_COLUMNS) + "\n")
        for r in tab["members"]:
            fh.write("\t".join(str(r[c]) for c in MEMBER_COLUMNS) + "\n")


def read_table(path):
    """the rows of variant_table.tsv or variant_members.tsv as write() wrote them: one dict per row, read counts and distances as integers"""
    with open(path) as fh:
        cols = fh.readline().rstrip("\n").lstrip("#").split("\t")
        return [{c: (v if c in _TEXT else int(v)) for c, v in zip(cols, line.rstrip("\n").split("\t"))} for line in fh if line.strip()]


def build(api, col, identity=DEFAULTS["identity"], max_dist=DEFAULTS["max_dist"], both_strands=True, wide_max_dist=DEFAULTS["wide_max_dist"]):
    """thresholds + ONE Api.near_pairs call (Api.near_pairs_wide when wide_max_dist is given) over the sequences of all samples + cluster + table -> the dict of
    table(), with variant_of / dist / strand [n] beside it"""
    seqs = col["seqs"]
    lengths = [len(s) for s in seqs]
    thr, K = thresholds(lengths, identity, max_dist, wide_max_dist)
    if len(seqs) > 1:
        near = api.near_pairs if wide_max_dist is None else api.near_pairs_wide
        pi, pj, dist, strand = near(ReadSet.from_strings(list(seqs)), K, both_strands=both_strands)
    else:
        pi = pj = dist = strand = np.zeros(0, dtype=np.int64)
    variant_of, centroids, mdist, mstrand = cluster(col["sizes"], lengths, seqs, (pi, pj), dist, thr, strand)
    tab = table(col, variant_of, centroids, mdist, mstrand)
    tab.update(variant_of=variant_of, dist=mdist, strand=mstrand)
    return tab


def check_args(args):
    """the range checks of the --variant_* flags -> an error text or None"""
    try:
        thresholds([], args.variant_identity, args.variant_max_dist, getattr(args, "variant_wide_max_dist", None))
    except ValueError as e:
        return str(e)
    return None


def add_flags(p):
    """the --variant_* flags, shared by the main command and the `variants` sub-command"""
    d = DEFAULTS
    p.add_argument('--variant_identity', type=str, default=d["identity"], help='extension: two consensuses are one variant when they differ by at most (1 - this) of the longer one\'s length in edits (a decimal fraction; the product is rounded down)')
    p.add_argument('--variant_max_dist', type=int, default=d["max_dist"], help='extension: ... and by at most this many edits (0..%d)' % NEAR_MAX_DIST)
    p.add_argument('--variant_wide_max_dist', type=int, default=d["wide_max_dist"], help='extension: when given, replaces --variant_max_dist as the edit bound (0..%d) and the comparison runs on the wide band kernels: for long amplicons or a low --variant_identity' % NEAR_WIDE_MAX_DIST)
    p.add_argument('--variant_one_strand', action='store_true', help='extension: compare the consensuses as they are, not also against their reverse complements')


def _kwargs(args):
    return dict(identity=args.variant_identity, max_dist=args.variant_max_dist, both_strands=not args.variant_one_strand, wide_max_dist=getattr(args, "variant_wide_max_dist", None))


def run(args, api, groups):
    """the --variants step: groups = [(sample name, folder, [(consensus id, n_reads, sequence)])].  The consensuses of ALL groups go through one Api.near_pairs call;
    <outfolder>/variants.fasta, variant_table.tsv and variant_members.tsv are written.  -> the dict of build()"""
    tab = build(api, collect(groups), **_kwargs(args))
    write(args.outfolder, tab)
    return tab


def variants_fasta(args, api=None):
    """the `variants` sub-command: every FASTA is one sample (named by its file name without the extension); read counts from names of this tool's consensuses
    (..._total_supporting_reads_N), 1 for any other name -> the three files in args.outfolder"""
    from . import runtime
    api = api or runtime.get_api()
    groups = []
    for path in args.fasta:
        q = classify.read_reference_fasta(path, unique_names=False)
        name = os.path.splitext(os.path.basename(path))[0]
        if any(name == g[0] for g in groups): raise ValueError("two FASTA files are both called %s: the sample names must differ" % name)
        groups.append((name, None, [(nm, classify.n_reads_of(nm) or 1, q.rs.get(i)[0]) for i, nm in enumerate(q.names)]))
    os.makedirs(args.outfolder, exist_ok=True)
    return run(args, api, groups)
