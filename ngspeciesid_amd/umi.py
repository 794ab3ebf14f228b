"""UMI mode (extension; sub-command `umi`): one consensus per original molecule.  The policy on top of ngsid_umi_pairs / ngsid_umi_centroids (include/ngsid_umi.h,
csrc/k_umi.hip), ngsid_demux_locate, ngsid_poa_consensus and ngsid_polish.

A UMI protocol flanks every template with a random tag at each end before PCR: adapter - flank - UMI - primer - amplicon - primer' - UMI' - flank'.  The reads of
one molecule share that pair of tags.  The library locates flanks, finds which keys lie within a few edits of each other and walks a pair list, and returns integers.
What a UMI is - the design, which end is which, the key of a read, the order of the centroids, the bins, their consensus and the files - is decided here.

Out of scope: chimera calls from one end's UMI shared by two bins, the combination with --fastq_dir / --demux_sheet, a cap on the reads per bin, and feeding the bin
consensuses into the variant table inside the run (`variants --fasta umi_consensus.fasta` does that)."""
from __future__ import annotations
import logging
import os
import numpy as np
from . import strand as _strand
from ._capi import ReadSet, UMI_MAX_LEN, UMI_MAX_DIST, DEMUX_MAX_TAG_LEN, POA_LOCAL, poa_params, polish_params

DEFAULTS = dict(umi_len=18, umi_len_slack=2, umi_max_dist=3, umi_flank_max_ed=3, umi_window=150, umi_min_reads=3, racon_iter=3)
ST_OK, ST_NO_UMI, ST_BAD_LEN, ST_SMALL_BIN = 0, 1, 2, 3
STATUS_NAMES = {ST_OK: "ok", ST_NO_UMI: "no_umi", ST_BAD_LEN: "bad_len", ST_SMALL_BIN: "small_bin"}
FLANKS = ("fwd_pre", "fwd_post", "rev_pre", "rev_post")
BIN_COLUMNS = ("bin", "umi", "reads", "distinct", "length")
READ_COLUMNS = ("read", "status", "strand", "umi", "bin", "dist")
_TAG_ALPHABET = frozenset("ACGTMRWSYKVHDBNX")           # demux.TAG_ALPHABET: ACGT + the IUPAC letters of the locator's equality rule
_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    _COMP[_a] = _b


class Design:
    """the four flanks of a UMI design, each 1 .. 64 letters over ACGT and the IUPAC codes: fwd_pre and fwd_post enclose the forward UMI at the head of a '+' read,
    rev_pre and rev_post the reverse UMI at the head of its reverse complement; umi_len letters per end, accepted within len_slack"""

    def __init__(self, fwd_pre, fwd_post, rev_pre, rev_post, umi_len=DEFAULTS["umi_len"], len_slack=DEFAULTS["umi_len_slack"]):
        self.fwd_pre, self.fwd_post, self.rev_pre, self.rev_post = fwd_pre, fwd_post, rev_pre, rev_post
        self.umi_len, self.len_slack = int(umi_len), int(len_slack)
        for name in FLANKS:
            tag = getattr(self, name)
            if not isinstance(tag, str) or not tag or not set(tag) <= _TAG_ALPHABET:
                raise ValueError("UMI flank %s = %r is outside the alphabet (upper-case ACGT and IUPAC codes)" % (name, tag))
            if len(tag) > DEMUX_MAX_TAG_LEN:
                raise ValueError("UMI flank %s of %d letters is longer than %d" % (name, len(tag), DEMUX_MAX_TAG_LEN))
        if self.len_slack < 0 or self.umi_len - self.len_slack < 1:
            raise ValueError("--umi_len_slack must be 0 .. --umi_len - 1, not %d with --umi_len %d" % (self.len_slack, self.umi_len))
        if 2 * (self.umi_len + self.len_slack) > UMI_MAX_LEN:
            raise ValueError("--umi_len + --umi_len_slack must be at most %d (a key of both ends holds %d letters), not %d" % (UMI_MAX_LEN // 2, UMI_MAX_LEN, self.umi_len + self.len_slack))

    def flanks(self):
        return [getattr(self, name) for name in FLANKS]


def seed_len(design: Design, max_dist):
    """the seed length of the neighbour search: the longest (at most 16, at least 4) at which the shortest accepted key still holds max_dist + 1 seeds"""
    return max(4, min(16, (2 * (design.umi_len - design.len_slack)) // (int(max_dist) + 1)))


def _window_slice(rs: ReadSet, r, side, a, b):
    """letters [a, b) of the side's window of read r: the read itself (side 0) or its reverse complement (side 1)"""
    o0, o1 = int(rs.off[r]), int(rs.off[r + 1])
    if side == 0:
        return rs.seq[o0 + a:o0 + b].tobytes().decode()
    return _COMP[rs.seq[o1 - b:o1 - a][::-1]].tobytes().decode()


def extract(api, rs: ReadSet, design: Design, window=DEFAULTS["umi_window"], flank_max_ed=DEFAULTS["umi_flank_max_ed"]):
    """four Api.demux_locate calls, one flank each -> dict(status uint8 [n] (ST_OK, ST_NO_UMI, ST_BAD_LEN), strand int8 [n] (0 '+', 1 '-', -1 none), key (list: the
    string u_fwd + u_rev or None), cut0 / cut1 int32 [n] (the inner cuts: post.end + 1 of side 0 and of side 1)).

    An end (side) carries a pair (pre, post) when both flanks are located there, pre.end < post.start and u = window[pre.end + 1 : post.start] has
    |len(u) - umi_len| <= len_slack.  '+': side 0 carries the forward pair and side 1 the reverse pair; '-': the other way round.  Both: the smaller sum of the four
    flank distances, a tie goes to '+'.  A read whose flanks are in place in some orientation but whose UMI length is off is bad_len, every other read without a
    key no_umi.  Each UMI is read in its own side's window coordinates, so both strands of one molecule give the same key."""
    n = rs.n
    H = [np.asarray(api.demux_locate(rs, [f], window=window, max_ed=flank_max_ed, iupac=True), dtype=np.int64).reshape(-1, 2, 5) if n else np.zeros((0, 2, 5), np.int64) for f in design.flanks()]
    status = np.full(n, ST_NO_UMI, dtype=np.uint8); strand = np.full(n, -1, dtype=np.int8)
    cut0 = np.zeros(n, dtype=np.int32); cut1 = np.zeros(n, dtype=np.int32)
    key = [None] * n

    def pair(pre, post, side):
        """-> (placed: both flanks located and in order, length of the UMI between them, sum of the two distances)"""
        placed = (pre[:, side, 0] >= 0) & (post[:, side, 0] >= 0) & (pre[:, side, 3] < post[:, side, 2])
        return placed, post[:, side, 2] - pre[:, side, 3] - 1, pre[:, side, 1] + post[:, side, 1]

    fits = lambda L: np.abs(L - design.umi_len) <= design.len_slack
    f0, lf0, ef0 = pair(H[0], H[1], 0); r1, lr1, er1 = pair(H[2], H[3], 1)          # '+'
    f1, lf1, ef1 = pair(H[0], H[1], 1); r0, lr0, er0 = pair(H[2], H[3], 0)          # '-'
    plus_placed, minus_placed = f0 & r1, f1 & r0
    plus = plus_placed & fits(lf0) & fits(lr1); minus = minus_placed & fits(lf1) & fits(lr0)
    take_minus = minus & (~plus | (ef1 + er0 < ef0 + er1))
    ok = plus | minus
    status[(plus_placed | minus_placed) & ~ok] = ST_BAD_LEN
    status[ok] = ST_OK
    strand[ok] = np.where(take_minus, 1, 0)[ok].astype(np.int8)
    for r in np.flatnonzero(ok).tolist():
        fs, rside = (1, 0) if take_minus[r] else (0, 1)
        u_f = _window_slice(rs, r, fs, int(H[0][r, fs, 3]) + 1, int(H[1][r, fs, 2]))
        u_r = _window_slice(rs, r, rside, int(H[2][r, rside, 3]) + 1, int(H[3][r, rside, 2]))
        key[r] = u_f + u_r
        post0, post1 = (H[3], H[1]) if take_minus[r] else (H[1], H[3])                 # the inner flank of side 0 and of side 1
        cut0[r] = int(post0[r, 0, 3]) + 1; cut1[r] = int(post1[r, 1, 3]) + 1
    return dict(status=status, strand=strand, key=key, cut0=cut0, cut1=cut1)


def bins(api, keys, max_dist=DEFAULTS["umi_max_dist"], min_reads=DEFAULTS["umi_min_reads"], design: Design | None = None):
    """keys: per read its key or None -> dict(umis [U] the distinct keys (ascending), counts int64 [U] their reads, key_of int64 [n] (-1: no key), bin_of int64 [U],
    centroids [B] (indices into umis, founding order), dist int64 [U] (edits to the bin's centroid), reads int64 [B], distinct int64 [B], small bool [B]: fewer than
    min_reads reads).  The distinct keys go through ONE Api.umi_pairs call at the design's seed length (every accepted key is then seedable) and one
    Api.umi_centroids call in the order of variants.cluster: reads descending, length descending, bytes ascending, index ascending."""
    if not 0 <= int(max_dist) <= UMI_MAX_DIST:
        raise ValueError("--umi_max_dist must be 0..%d, not %d" % (UMI_MAX_DIST, int(max_dist)))
    umis = sorted({k for k in keys if k is not None})
    index = {k: i for i, k in enumerate(umis)}
    key_of = np.array([index[k] if k is not None else -1 for k in keys], dtype=np.int64).reshape(-1)
    U = len(umis)
    counts = np.bincount(key_of[key_of >= 0], minlength=U).astype(np.int64)
    lens = np.array([len(k) for k in umis], dtype=np.int64)
    g = seed_len(design, max_dist) if design is not None else max(4, min(16, (int(lens.min()) if U else 16) // (int(max_dist) + 1)))
    if U > 1:
        pi, pj, pd = api.umi_pairs(ReadSet.from_strings(umis), int(max_dist), g)
    else:
        pi = pj = np.zeros(0, dtype=np.uint32); pd = np.zeros(0, dtype=np.uint8)
    order = np.lexsort((np.arange(U), -lens, -counts))               # the keys are distinct and ascending: the index stands for the bytes
    bin_of, cent = api.umi_centroids(pi, pj, order)
    bin_of = np.asarray(bin_of, dtype=np.int64); cent = np.asarray(cent, dtype=np.int64)
    B = len(cent)
    dist = np.zeros(U, dtype=np.int64)
    if U:
        c = cent[bin_of]; x = np.arange(U)
        member = np.flatnonzero(c != x)
        code = np.asarray(pi, dtype=np.int64) * U + np.asarray(pj, dtype=np.int64)   # ascending: the pairs come in (i, j) order
        want = np.minimum(x, c)[member] * U + np.maximum(x, c)[member]
        dist[member] = np.asarray(pd, dtype=np.int64)[np.searchsorted(code, want)]
    reads = np.bincount(bin_of, weights=counts, minlength=B).astype(np.int64) if U else np.zeros(0, dtype=np.int64)
    distinct = np.bincount(bin_of, minlength=B).astype(np.int64) if U else np.zeros(0, dtype=np.int64)
    return dict(umis=umis, counts=counts, key_of=key_of, bin_of=bin_of, centroids=cent.tolist(), dist=dist, reads=reads, distinct=distinct, small=reads < int(min_reads),
                seed_len=g, n_pairs=int(len(pi)))


def trimmed_oriented(rs: ReadSet, ex):
    """the reads cut at their inner cuts (read[cut0 : L - cut1] for the reads with a key, whole otherwise) and the '-' reads reverse-complemented: the amplicons,
    all on the forward strand"""
    from . import demux
    ok = ex["status"] == ST_OK
    return _strand.orient_reads(demux._trimmed(rs, ex["cut0"], ex["cut1"], ok), ok & (ex["strand"] == 1))


def bin_groups(bn, keep=None):
    """-> (bins kept [G] (all bins that are not small, ascending, or `keep`), read lists [G]: the reads of each, ascending)"""
    kept = [b for b in range(len(bn["centroids"])) if not bn["small"][b]] if keep is None else list(keep)
    bin_of_read = np.where(bn["key_of"] >= 0, bn["bin_of"][np.maximum(bn["key_of"], 0)], -1) if len(bn["bin_of"]) else np.full(len(bn["key_of"]), -1, dtype=np.int64)
    order = np.argsort(bin_of_read, kind="stable")
    start = np.searchsorted(bin_of_read[order], np.arange(len(bn["centroids"]) + 1))
    return kept, [order[start[b]:start[b + 1]].astype(np.uint32) for b in kept]


def consensus_params(racon_iter=DEFAULTS["racon_iter"]):
    """the draft and polishing parameters: those of pipeline._consensus_stages at its defaults"""
    from . import pipeline
    draft = poa_params(mode=POA_LOCAL, match=5, mismatch=-4, gap=-2, tile_depth=pipeline.TILE_DEPTH, band=0, node_cap=0, trim=pipeline.DRAFT_TRIM, single_below=pipeline.SINGLE_BELOW)
    polish = polish_params(iters=int(racon_iter), k=13, w=20, tile_depth=pipeline.TILE_DEPTH, band=0, node_cap=0, trim=2, aln_mode=2, stop_when_stable=True, single_below=pipeline.SINGLE_BELOW)
    return draft, polish


def consensus(api, work: ReadSet, lists, racon_iter=DEFAULTS["racon_iter"]):
    """work = trimmed_oriented(...), lists = the read lists of bin_groups -> (drafts [G], polished [G]): ONE Api.poa_consensus call with the bins as groups, then one
    Api.polish call with racon_iter rounds (polished = drafts when racon_iter is 0)"""
    if not lists:
        return [], []
    from .pipeline import group_offsets
    draft_prm, polish_prm = consensus_params(racon_iter)
    go, ro = group_offsets(lists), np.concatenate(lists)
    drafts = list(api.poa_consensus(work, go, draft_prm, read_order=ro))
    if int(racon_iter) <= 0:
        return drafts, list(drafts)
    pol, _ = api.polish(ReadSet.from_strings(drafts), work, go, polish_prm, read_order=ro)
    return drafts, list(pol)


def run(api, rs: ReadSet, design: Design, window=DEFAULTS["umi_window"], flank_max_ed=DEFAULTS["umi_flank_max_ed"], max_dist=DEFAULTS["umi_max_dist"],
        min_reads=DEFAULTS["umi_min_reads"], racon_iter=DEFAULTS["racon_iter"], timings=None):
    """extract + bins + consensus -> dict(extract, bins, kept (the bins with a consensus), lists, drafts, polished, status uint8 [n] with ST_SMALL_BIN for the reads
    of bins below min_reads, bin int64 [n] (-1: none), dist int64 [n])"""
    from time import perf_counter
    T = {} if timings is None else timings
    t0 = perf_counter()
    ex = extract(api, rs, design, window, flank_max_ed)
    T["extract"] = perf_counter() - t0; t0 = perf_counter()
    bn = bins(api, ex["key"], max_dist, min_reads, design)
    T["bins"] = perf_counter() - t0; t0 = perf_counter()
    kept, lists = bin_groups(bn)
    work = trimmed_oriented(rs, ex) if kept else rs
    T["orient"] = perf_counter() - t0; t0 = perf_counter()
    drafts, _ = consensus(api, work, lists, 0)
    T["consensus"] = perf_counter() - t0; t0 = perf_counter()
    polished = list(drafts)
    if kept and int(racon_iter) > 0:
        from .pipeline import group_offsets
        polished = list(api.polish(ReadSet.from_strings(drafts), work, group_offsets(lists), consensus_params(racon_iter)[1], read_order=np.concatenate(lists))[0])
    T["polish"] = perf_counter() - t0
    has = bn["key_of"] >= 0
    kk = np.maximum(bn["key_of"], 0)
    rbin = np.where(has, bn["bin_of"][kk], -1) if len(bn["bin_of"]) else np.full(rs.n, -1, dtype=np.int64)
    rdist = np.where(has, bn["dist"][kk], 0) if len(bn["bin_of"]) else np.zeros(rs.n, dtype=np.int64)
    status = ex["status"].copy()
    if len(bn["small"]):
        status[has & bn["small"][np.maximum(rbin, 0)]] = ST_SMALL_BIN
    return dict(extract=ex, bins=bn, kept=kept, lists=lists, drafts=drafts, polished=polished, status=status, bin=rbin, dist=rdist, timings=T)


def write(outfolder, names, res):
    """umi_consensus.fasta (`>umi_{b};reads={n};umi={key}`, the polished sequence of every bin with at least min_reads reads), umi_bins.tsv (BIN_COLUMNS, every
    bin), umi_reads.tsv (READ_COLUMNS, every read) and umi_summary.tsv (one row per status); tab-separated, one header line starting with '#'.  names: a list of
    read names or an object with .get(i)"""
    bn, ex = res["bins"], res["extract"]
    name = names.get if hasattr(names, "get") else names.__getitem__
    first_word = lambda h: h.split()[0] if h.split() else h
    length = {b: len(s) for b, s in zip(res["kept"], res["polished"])}
    with open(os.path.join(outfolder, "umi_consensus.fasta"), "w") as fh:
        for b, s in zip(res["kept"], res["polished"]):
            fh.write(">umi_%d;reads=%d;umi=%s\n%s\n" % (b, int(bn["reads"][b]), bn["umis"][bn["centroids"][b]], s))
    with open(os.path.join(outfolder, "umi_bins.tsv"), "w") as fh:
        fh.write("#" + "\t".join(BIN_COLUMNS) + "\n")
        for b, c in enumerate(bn["centroids"]):
            fh.write("umi_%d\t%s\t%d\t%d\t%d\n" % (b, bn["umis"][c], int(bn["reads"][b]), int(bn["distinct"][b]), length.get(b, 0)))
    with open(os.path.join(outfolder, "umi_reads.tsv"), "w") as fh:
        fh.write("#" + "\t".join(READ_COLUMNS) + "\n")
        for r in range(len(res["status"])):
            k = ex["key"][r]
            fh.write("%s\t%s\t%s\t%s\t%s\t%d\n" % (first_word(name(r)), STATUS_NAMES[int(res["status"][r])], "+-"[int(ex["strand"][r])] if ex["strand"][r] >= 0 else ".",
                                                   k if k is not None else ".", "umi_%d" % int(res["bin"][r]) if res["bin"][r] >= 0 else ".", int(res["dist"][r])))
    with open(os.path.join(outfolder, "umi_summary.tsv"), "w") as fh:
        fh.write("#status\treads\n")
        for st in sorted(STATUS_NAMES):
            fh.write("%s\t%d\n" % (STATUS_NAMES[st], int((res["status"] == st).sum())))


def read_table(path):
    """the rows of one of the three tables as write() wrote them: one dict per row, counts as integers"""
    text = ("bin", "umi", "read", "status", "strand")
    with open(path) as fh:
        cols = fh.readline().rstrip("\n").lstrip("#").split("\t")
        return [{c: (v if c in text else int(v)) for c, v in zip(cols, line.rstrip("\n").split("\t"))} for line in fh if line.strip()]


def add_flags(p):
    """the flags of the `umi` sub-command"""
    d = DEFAULTS
    p.add_argument('--umi_fwd', type=str, required=True, help='PRE,POST: the two flanks that enclose the forward UMI, as they read at the head of a forward read (up to %d letters each, IUPAC codes allowed)' % DEMUX_MAX_TAG_LEN)
    p.add_argument('--umi_rev', type=str, required=True, help='PRE,POST: the two flanks that enclose the reverse UMI, as they read at the head of the reverse complement of a forward read')
    p.add_argument('--umi_len', type=int, default=d["umi_len"], help='letters of the UMI at each end')
    p.add_argument('--umi_len_slack', type=int, default=d["umi_len_slack"], help='a UMI is accepted when its length is within this of --umi_len')
    p.add_argument('--umi_max_dist', type=int, default=d["umi_max_dist"], help='two keys (forward + reverse UMI) belong to one molecule within this many edits (0..%d)' % UMI_MAX_DIST)
    p.add_argument('--umi_flank_max_ed', type=int, default=d["umi_flank_max_ed"], help='largest edit distance at which a flank counts as found in a read end')
    p.add_argument('--umi_window', type=int, default=d["umi_window"], help='letters of each read end that are searched for the flanks (1..256)')
    p.add_argument('--umi_min_reads', type=int, default=d["umi_min_reads"], help='a bin gets a consensus from this many reads on')
    p.add_argument('--racon_iter', type=int, default=d["racon_iter"], help='polishing rounds of every bin consensus (0: the draft)')


def design_of(args) -> Design:
    def two(text, flag):
        f = [x.strip() for x in str(text).split(",")]
        if len(f) != 2:
            raise ValueError("%s takes two flanks as PRE,POST, not %r" % (flag, text))
        return f
    fp, fq = two(args.umi_fwd, "--umi_fwd"); rp, rq = two(args.umi_rev, "--umi_rev")
    return Design(fp, fq, rp, rq, args.umi_len, args.umi_len_slack)


def check_args(args):
    """the range checks of the `umi` flags -> an error text or None"""
    try:
        design_of(args)
    except ValueError as e:
        return str(e)
    if not 0 <= args.umi_max_dist <= UMI_MAX_DIST:
        return "--umi_max_dist must be 0..%d, not %d" % (UMI_MAX_DIST, args.umi_max_dist)
    if not 1 <= args.umi_window <= 256:
        return "--umi_window must be 1..256, not %d" % args.umi_window
    if args.umi_flank_max_ed < 0:
        return "--umi_flank_max_ed must not be negative"
    if args.umi_min_reads < 1:
        return "--umi_min_reads must be at least 1"
    if args.racon_iter < 0:
        return "--racon_iter must not be negative"
    return None


def umi_fastq(args, api=None):
    """the `umi` sub-command: one FASTQ in, the four files of write() in args.outfolder -> the dict of run()"""
    from . import fastio, runtime
    api = api or runtime.get_api()
    names, rs, _ = fastio.read_fastq(args.fastq)
    work = rs
    if rs.n and fastio.count_foreign_bases(rs.seq):
        seq = rs.seq.copy()
        changed = fastio.normalize_bases(seq)
        logging.warning("%d bases outside A/C/G/T/N are read as upper case / N", changed)
        work = ReadSet(seq, rs.qual, rs.off)
    res = run(api, work, design_of(args), window=args.umi_window, flank_max_ed=args.umi_flank_max_ed, max_dist=args.umi_max_dist, min_reads=args.umi_min_reads, racon_iter=args.racon_iter)
    os.makedirs(args.outfolder, exist_ok=True)
    write(args.outfolder, names, res)
    return res
