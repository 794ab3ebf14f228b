"""Recruit every read of a sample to its nearest final consensus (extension; include/ngsid_recruit.h, csrc/k_recruit.hip).

A consensus' read count (total_supporting_reads) is the size of the greedy clusters pooled into it: a lower bound.  Reads of clusters below --abundance_ratio, singletons
and reads whose cluster had a bad representative support nothing, although most of them are reads of one of the final sequences.  Api.recruit locates every read inside
every final consensus of its sample (the consensus end to end, the read's primers, tags and adapter remains free) on both strands and returns the two nearest per read
as integers; what they mean is decided here:
  thresholds  the edit bound of a consensus of m letters: floor((1 - min_identity) * m); by default min_identity = 1 - 10^(-q / 10) of the run's --q, the expected-error
              bound every kept read has already passed (0.80 at the default 7.0)
  assign      per read: assigned; ambiguous when a second consensus hits within min_margin edits of the best (the default 1 calls only exact ties ambiguous); unassigned
  recount     per centre reads_clustered (its count today), reads_recruited and where the recruited reads came from: the centre's own clusters, clusters of another centre,
              clusters below the cut-off or singletons; per sample the ambiguous and unassigned totals
  run         the above for one sample or many, ONE Api.recruit call
and the two tables of `--consensus --recruit` / the `recruit` sub-command (recount.tsv, read_assignments.tsv)."""
from __future__ import annotations
import math
import numpy as np
from ._capi import ReadSet, RECRUIT_MAX_LEN

UNASSIGNED, ASSIGNED, AMBIGUOUS = 0, 1, 2
STATUS_NAMES = ("unassigned", "assigned", "ambiguous")
RECOUNT_COLUMNS = ("reads_clustered", "reads_recruited", "from_own_clusters", "from_other_centres", "from_unclustered")


def default_min_identity(q=7.0) -> float:
    """1 - 10^(-q / 10): the expected-error bound of the read filter (--q)"""
    return 1.0 - 10.0 ** (-float(q) / 10.0)


def thresholds(lengths, min_identity=None, q=7.0) -> np.ndarray:
    """floor((1 - min_identity) * m) per consensus length m -> int32.  (The product is taken with a 1e-9 guard, so that 0.2 * 5 is 1 and not floor(0.9999999999999998).)"""
    mi = default_min_identity(q) if min_identity is None else float(min_identity)
    if not 0.0 <= mi <= 1.0:
        raise ValueError("min_identity is a fraction in [0, 1]")
    return np.array([int(math.floor((1.0 - mi) * int(m) + 1e-9)) for m in lengths], dtype=np.int32)


def assign(hits, min_margin=1) -> np.ndarray:
    """status per read (int8: UNASSIGNED, ASSIGNED, AMBIGUOUS) of a hit array in RECRUIT_FIELDS order"""
    h = np.asarray(hits).reshape(-1, 6)
    st = np.where(h[:, 0] >= 0, ASSIGNED, UNASSIGNED).astype(np.int8)
    st[(h[:, 0] >= 0) & (h[:, 5] >= 0) & (h[:, 5] - h[:, 1] < int(min_margin))] = AMBIGUOUS
    return st


def recount(hits, status, n_centres, origin, clustered=None) -> dict:
    """one sample: hits with centre numbers local to the sample, status of assign, origin[r] = the centre whose pooled clusters hold read r, or -1 (a cluster below the
    cut-off, a singleton, a read that was not clustered); clustered = the centres' counts today (default: the reads origin gives them) ->
    dict(centres = one dict of RECOUNT_COLUMNS per centre, ambiguous, unassigned)"""
    h = np.asarray(hits).reshape(-1, 6); st = np.asarray(status); og = np.asarray(origin, dtype=np.int64)
    if not (len(h) == len(st) == len(og)):
        raise ValueError("recount: hits, status and origin hold one entry per read")
    got = st == ASSIGNED
    centres = []
    for c in range(int(n_centres)):
        mine = got & (h[:, 0] == c)
        centres.append(dict(reads_clustered=int((og == c).sum()) if clustered is None else int(clustered[c]), reads_recruited=int(mine.sum()),
                            from_own_clusters=int((mine & (og == c)).sum()), from_other_centres=int((mine & (og >= 0) & (og != c)).sum()),
                            from_unclustered=int((mine & (og < 0)).sum())))
    return dict(centres=centres, ambiguous=int((st == AMBIGUOUS).sum()), unassigned=int((st == UNASSIGNED).sum()))


def run(api, rs: ReadSet, seg_off, seqs_per_sample, origins=None, clustered=None, min_identity=None, q=7.0, min_margin=1, both_strands=True):
    """reads [seg_off[s], seg_off[s + 1]) of rs against the final sequences seqs_per_sample[s], ONE Api.recruit call for all samples -> one dict(hits [n_s, 6] with
    centre numbers local to the sample, status, counts = recount(...)) per sample.  origins[s] / clustered[s]: the arguments of recount (default: nothing is clustered)."""
    so = np.asarray(seg_off, dtype=np.int64); ns = len(so) - 1
    if len(seqs_per_sample) != ns:
        raise ValueError("recruit.run: one list of sequences per sample")
    flat = [q_ for seqs in seqs_per_sample for q_ in seqs]
    for q_ in flat:
        if len(q_) > RECRUIT_MAX_LEN:
            raise ValueError("recruit: a consensus of %d letters (at most %d)" % (len(q_), RECRUIT_MAX_LEN))
    cons_off = np.concatenate(([0], np.cumsum([len(seqs) for seqs in seqs_per_sample]))).astype(np.uint64)
    bound = thresholds([len(q_) for q_ in flat], min_identity, q)
    hits = api.recruit(rs, so.astype(np.uint64), ReadSet.from_strings(flat), cons_off, bound, both_strands=both_strands)
    out = []
    for s in range(ns):
        h = hits[int(so[s]):int(so[s + 1])].copy()
        base = np.int32(cons_off[s])
        for f in (0, 4):
            h[:, f] = np.where(h[:, f] >= 0, h[:, f] - base, -1)
        st = assign(h, min_margin)
        n = len(h)
        og = np.full(n, -1, dtype=np.int64) if origins is None or origins[s] is None else origins[s]
        out.append(dict(hits=h, status=st, counts=recount(h, st, len(seqs_per_sample[s]), og, None if clustered is None else clustered[s])))
    return out


def nothing(n_reads) -> dict:
    """the result of a sample without a final sequence: every read unassigned"""
    h = np.full((int(n_reads), 6), -1, dtype=np.int32); h[:, 2] = 0
    st = assign(h)
    return dict(hits=h, status=st, counts=recount(h, st, 0, np.full(int(n_reads), -1, dtype=np.int64)))


def origin_of(n_reads, lists) -> np.ndarray:
    """origin for recount: lists[c] = the reads (numbers local to the sample) of the clusters pooled into centre c; a read listed twice stays with the first centre"""
    og = np.full(int(n_reads), -1, dtype=np.int64)
    for c, l in enumerate(lists):
        l = np.asarray(l, dtype=np.int64)
        l = l[og[l] < 0]
        og[l] = c
    return og


# ---- the command line
def add_flags(p):
    p.add_argument('--recruit_min_identity', type=float, default=None, help='extension: a read counts for a consensus of m letters when the consensus lies inside it within floor((1 - this) * m) edits (default: 1 - 10^(-q / 10) of --q, the expected-error bound every kept read has passed: 0.80 at --q 7)')
    p.add_argument('--recruit_min_margin', type=int, default=1, help='extension: a read is ambiguous when its second-nearest consensus is fewer than this many edits behind its nearest (1: exact ties only)')
    p.add_argument('--recruit_one_strand', action='store_true', help='extension: compare the reads with the forward strand of every consensus only')


def check_args(args):
    mi = getattr(args, "recruit_min_identity", None)
    if mi is not None and not 0.0 <= mi <= 1.0:
        return "--recruit_min_identity is a fraction in [0, 1]."
    if getattr(args, "recruit_min_margin", 1) < 0:
        return "--recruit_min_margin must not be negative."
    return None


def policy_from_args(args) -> dict:
    return dict(min_identity=getattr(args, "recruit_min_identity", None), q=getattr(args, "quality_threshold", 7.0), min_margin=getattr(args, "recruit_min_margin", 1),
                both_strands=not getattr(args, "recruit_one_strand", False))


def write_sample(folder, names, ids, seqs, res):
    """recount.tsv and read_assignments.tsv of one sample into its folder"""
    import os
    write_recount(os.path.join(folder, "recount.tsv"), ids, res["counts"])
    write_assignments(os.path.join(folder, "read_assignments.tsv"), names, res["hits"], res["status"], ids, [len(q_) for q_ in seqs])


def recruit_fastq(args, api=None):
    """the `recruit` sub-command: the reads of --fastq against the sequences of --fasta, taken as one sample -> <outfolder>/recount.tsv, read_assignments.tsv.  A consensus
    is named by the first word of its header; reads_clustered is read from names of this tool's consensuses (..._total_supporting_reads_N), else 0; nothing is known of the
    clusters, so every recruited read counts as from_unclustered."""
    import os, re
    from . import runtime
    from .help_functions import readfq
    api = api or runtime.get_api()
    with open(args.fasta) as fh:
        cons = [(name.split()[0] if name.split() else "", sq[0].upper()) for name, sq in readfq(fh)]
    with open(args.fastq) as fh:
        reads = [(name.split()[0] if name.split() else "", sq[0].upper()) for name, sq in readfq(fh)]
    ids = [c[0] for c in cons]; seqs = [c[1] for c in cons]
    clustered = [int(m.group(1)) if m else 0 for m in (re.search(r"_total_supporting_reads_(\d+)", i) for i in ids)]
    res = run(api, ReadSet.from_strings([r[1] for r in reads]), [0, len(reads)], [seqs], None, [clustered], **policy_from_args(args))[0]
    os.makedirs(args.outfolder, exist_ok=True)
    write_sample(args.outfolder, [r[0] for r in reads], ids, seqs, res)
    return res


# ---- the tables
def write_recount(path, ids, counts, sample=None, header=True, mode="w"):
    """recount.tsv: one row per consensus (ids[c] = its id as in the file names) with RECOUNT_COLUMNS, then the sample's ambiguous and unassigned totals as comment
    lines; sample: a leading column (recount_all.tsv)"""
    lead = [] if sample is None else ["sample"]
    with open(path, mode) as f:
        if header:
            f.write("\t".join(lead + ["consensus"] + list(RECOUNT_COLUMNS)) + "\n")
        for cid, c in zip(ids, counts["centres"]):
            f.write("\t".join(([] if sample is None else [str(sample)]) + [str(cid)] + [str(c[k]) for k in RECOUNT_COLUMNS]) + "\n")
        tag = "" if sample is None else "\t%s" % sample
        f.write("#ambiguous%s\t%d\n#unassigned%s\t%d\n" % (tag, counts["ambiguous"], tag, counts["unassigned"]))


def write_assignments(path, names, hits, status, ids, lengths):
    """read_assignments.tsv: read, consensus, strand, ed, identity = 1 - ed / m, status; '-' where the read has no consensus"""
    with open(path, "w") as f:
        f.write("read\tconsensus\tstrand\ted\tidentity\tstatus\n")
        for nm, h, st in zip(names, np.asarray(hits).reshape(-1, 6).tolist(), np.asarray(status).tolist()):
            if h[0] < 0:
                f.write("%s\t-\t-\t-\t-\t%s\n" % (nm, STATUS_NAMES[st]))
            else:
                f.write("%s\t%s\t%s\t%d\t%.4f\t%s\n" % (nm, ids[h[0]], "+-"[h[2]], h[1], 1.0 - h[1] / float(lengths[h[0]]), STATUS_NAMES[st]))
