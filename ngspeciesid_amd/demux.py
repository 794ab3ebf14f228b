"""Demultiplexing of a pooled run (extension; `--demux_sheet`): the policy on top of ngsid_demux_locate (include/ngsid_demux.h, csrc/k_demux.hip).

The library locates every sample tag in both end windows of every read and returns integers.  Which read goes to which sample - the sheet, the margin
between the best and the second-best tag, the strand rule, the cuts - is decided here, and the files a demultiplexer leaves are written here:
<outfolder>/demux/<sample>.fastq, <outfolder>/demux_unassigned.fastq, <outfolder>/demux_summary.tsv.

`--demux_mid_tags discard | split`: the whole read is scanned for the sheet's tags on both strands (ngsid_demux_scan, csrc/k_demux_scan.hip); a read with a tag inside
is a concatemer and is discarded or cut into pieces that are demultiplexed once more (+ <outfolder>/demux_concatemers.tsv).
"""
from __future__ import annotations
import ctypes as C
import logging
import os
import numpy as np
from . import fastio, runtime
from ._capi import ReadSet, DEMUX_MAX_TAG_LEN

TAG_ALPHABET = frozenset("ACGTMRWSYKVHDBNX")          # ACGT + the IUPAC letters of the locator's equality rule (csrc/host_io.hip iupac_eq)
ST_ASSIGNED, ST_NO_TAG, ST_AMBIGUOUS, ST_NOT_IN_SHEET, ST_EMPTY = 0, 1, 2, 3, 4
STATUS_NAMES = {ST_NO_TAG: "no_tag", ST_AMBIGUOUS: "ambiguous", ST_NOT_IN_SHEET: "pair_not_in_sheet", ST_EMPTY: "nothing_left"}


class Sheet:
    """samples [S] (names), tags [T] (unique tag strings), fwd [S] / rev [S] (tag indices; rev is None for a single-ended kit)"""

    def __init__(self, samples, tags, fwd, rev):
        self.samples, self.tags = list(samples), list(tags)
        self.fwd = np.asarray(fwd, dtype=np.int32); self.rev = None if rev is None else np.asarray(rev, dtype=np.int32)

    @property
    def dual(self):
        return self.rev is not None


def _plain_file_name(name):
    return bool(name) and name not in (".", "..") and os.path.basename(name) == name and "/" not in name and "\\" not in name and "\0" not in name and name == name.strip()


def read_sheet(path) -> Sheet:
    """TSV, one row per sample: sample<TAB>forward tag[<TAB>reverse tag]; '#' lines and blank lines are skipped.  The third column is empty or absent on every row
    (single-ended kit) or present on every row (dual kit).  Identical tag strings share one tag index.  ValueError names the offending row."""
    samples, fwd, rev, tags, index = [], [], [], [], {}
    pairs = {}
    dual = None

    def tag_index(tag, row):
        if not tag or not set(tag) <= TAG_ALPHABET:
            raise ValueError("%s, row %d: tag %r is outside the alphabet (upper-case ACGT and IUPAC codes)" % (path, row, tag))
        if len(tag) > DEMUX_MAX_TAG_LEN:
            raise ValueError("%s, row %d: tag of %d bases is longer than %d" % (path, row, len(tag), DEMUX_MAX_TAG_LEN))
        if tag not in index:
            index[tag] = len(tags); tags.append(tag)
        return index[tag]

    with open(path) as fh:
        for row, line in enumerate(fh, 1):
            line = line.rstrip("\r\n")
            if not line.strip() or line.startswith("#"):
                continue
            f = line.split("\t")
            if len(f) < 2 or len(f) > 3:
                raise ValueError("%s, row %d: expected sample<TAB>forward tag[<TAB>reverse tag]" % (path, row))
            name, ftag, rtag = f[0], f[1].strip(), (f[2].strip() if len(f) == 3 else "")
            if not _plain_file_name(name):
                raise ValueError("%s, row %d: sample name %r is not a plain file name" % (path, row, name))
            if name in samples:
                raise ValueError("%s, row %d: sample name %r is listed twice" % (path, row, name))
            if dual is None:
                dual = bool(rtag)
            elif dual != bool(rtag):
                raise ValueError("%s, row %d: the reverse tag is present on some rows and missing on others" % (path, row))
            a = tag_index(ftag, row); b = tag_index(rtag, row) if dual else -1
            if (a, b) in pairs:
                raise ValueError("%s, row %d: sample %r has the tags of sample %r" % (path, row, name, samples[pairs[(a, b)]]))
            if dual and (b, a) in pairs and a != b:
                raise ValueError("%s, row %d: the tags of sample %r are those of sample %r the other way round" % (path, row, name, samples[pairs[(b, a)]]))
            pairs[(a, b)] = len(samples)
            samples.append(name); fwd.append(a); rev.append(b)
    if not samples:
        raise ValueError("%s: no sample row" % path)
    return Sheet(samples, tags, fwd, rev if dual else None)


def assign(hits, sheet: Sheet, min_margin, lens=None):
    """hits [n, 2, 5] of Api.demux_locate -> (sample [n] int32 or -1, strand [n] int8 or -1, status [n] uint8, cut0 [n], cut1 [n] int32).

    A side's hit is valid if tag >= 0 and (ed2 < 0 or ed2 - ed >= min_margin).  Dual sheet: the valid tags (a, b) of sides 0 and 1 are a sample's (forward, reverse)
    -> strand 0, or its (reverse, forward) -> strand 1.  Single-ended sheet: a valid tag on side 0 and no tag at all on side 1 -> strand 0, the mirror image ->
    strand 1.  Status: 0 assigned, 1 a needed end has no tag, 2 a needed end is ambiguous by the margin, 3 the pair is not in the sheet (single-ended: both ends
    carry a tag), 4 nothing is left after trimming (lens given and cut0 + cut1 >= L).  cut = end + 1 of each side that carried a tag: the kept read is
    read[cut0 : L - cut1] (side 1 counts from the tail: its positions are those of the reverse complement)."""
    h = np.asarray(hits, dtype=np.int32).reshape(-1, 2, 5)
    n = len(h)
    tag, ed, end, ed2 = h[:, :, 0], h[:, :, 1], h[:, :, 3], h[:, :, 4]
    has = tag >= 0
    valid = has & ((ed2 < 0) | (ed2 - ed >= int(min_margin)))
    cut = np.where(has, end + 1, 0).astype(np.int32)
    sample = np.full(n, -1, dtype=np.int32); strand = np.full(n, -1, dtype=np.int8); status = np.zeros(n, dtype=np.uint8)
    T = len(sheet.tags)
    if sheet.dual:
        table = np.full((T, T), -1, dtype=np.int32)                   # [tag of side 0][tag of side 1] -> sample * 2 + strand
        for s, (a, b) in enumerate(zip(sheet.fwd.tolist(), sheet.rev.tolist())):
            if table[b, a] < 0: table[b, a] = 2 * s + 1
            table[a, b] = 2 * s
        none = ~has[:, 0] | ~has[:, 1]
        amb = ~none & (~valid[:, 0] | ~valid[:, 1])
        ok = ~none & ~amb
        code = np.full(n, -1, dtype=np.int32)
        code[ok] = table[tag[ok, 0], tag[ok, 1]]
    else:
        owner = np.full(T, -1, dtype=np.int32); owner[sheet.fwd] = np.arange(len(sheet.samples), dtype=np.int32)
        none = ~has[:, 0] & ~has[:, 1]
        both = has[:, 0] & has[:, 1]
        side = np.where(has[:, 1] & ~has[:, 0], 1, 0)                  # the one side that carries a tag
        one = ~none & ~both
        amb = one & ~valid[np.arange(n), side]
        ok = one & ~amb
        code = np.full(n, -1, dtype=np.int32)
        code[ok] = 2 * owner[tag[np.arange(n), side][ok]] + side[ok]
    found = code >= 0
    sample[found] = code[found] >> 1; strand[found] = (code[found] & 1).astype(np.int8)
    status[~found] = ST_NOT_IN_SHEET; status[amb] = ST_AMBIGUOUS; status[none] = ST_NO_TAG
    if lens is not None:
        gone = found & (cut[:, 0].astype(np.int64) + cut[:, 1] >= np.asarray(lens, dtype=np.int64))
        status[gone] = ST_EMPTY; sample[gone] = -1; strand[gone] = -1
    return sample, strand, status, cut[:, 0].copy(), cut[:, 1].copy()


def _trimmed(rs: ReadSet, cut0, cut1, keep):
    """the reads with read[cut0 : L - cut1] for the reads `keep`, whole otherwise (bases and qualities), as a read set of its own"""
    off = rs.off.astype(np.int64); lens = np.diff(off)
    c0 = np.where(keep, cut0, 0).astype(np.int64); c1 = np.where(keep, cut1, 0).astype(np.int64)
    nl = np.maximum(lens - c0 - c1, 0)
    noff = np.zeros(len(lens) + 1, dtype=np.uint64); noff[1:] = np.cumsum(nl)
    total = int(noff[-1])
    seq = np.empty(max(total, 1), dtype=np.uint8)[:total]; qual = np.empty(max(total, 1), dtype=np.uint8)[:total]
    if len(lens):
        lib = runtime.load_library()
        so = np.ascontiguousarray(off[:-1] + c0, dtype=np.uint64); ln = np.ascontiguousarray(nl, dtype=np.uint32); do = np.ascontiguousarray(noff[:-1])
        lib.ngsid_host_gather(fastio._p(rs.seq), fastio._p(so), fastio._p(ln), C.c_uint64(len(ln)), fastio._p(seq), fastio._p(do))
        lib.ngsid_host_gather(fastio._p(rs.qual), fastio._p(so), fastio._p(ln), C.c_uint64(len(ln)), fastio._p(qual), fastio._p(do))
    return ReadSet(seq, qual, noff)


def write_outputs(outfolder, sheet: Sheet, names, rs: ReadSet, hits, result, keep_tags=False):
    """demux/<sample>.fastq (samples with reads only; input order, headers unchanged, tags cut unless keep_tags), demux_unassigned.fastq (whole reads) and
    demux_summary.tsv -> the folder of the sample files"""
    sample, strand, status, cut0, cut1 = result
    folder = os.path.join(outfolder, "demux")
    os.makedirs(folder, exist_ok=True)
    for f in os.listdir(folder):                                       # sample files of an earlier run are not samples of this one
        if f.endswith((".fastq", ".fq")) and os.path.isfile(os.path.join(folder, f)):
            os.remove(os.path.join(folder, f))
    assigned = sample >= 0
    out = rs if keep_tags else _trimmed(rs, cut0, cut1, assigned)
    for s, name in enumerate(sheet.samples):
        idx = np.flatnonzero(sample == s)
        if len(idx):
            fastio.write_fastq(os.path.join(folder, name + ".fastq"), idx, names, out)
    fastio.write_fastq(os.path.join(outfolder, "demux_unassigned.fastq"), np.flatnonzero(~assigned), names, out)
    h = np.asarray(hits, dtype=np.int32).reshape(-1, 2, 5)
    tag_ed = np.where(h[:, :, 0] >= 0, h[:, :, 1], 0).sum(axis=1)
    with open(os.path.join(outfolder, "demux_summary.tsv"), "w") as fh:
        fh.write("#sample\treads\tstrand0\tstrand1\ttag_ed_sum\n")
        for s, name in enumerate(sheet.samples):
            m = sample == s
            fh.write("%s\t%d\t%d\t%d\t%d\n" % (name, int(m.sum()), int((m & (strand == 0)).sum()), int((m & (strand == 1)).sum()), int(tag_ed[m].sum())))
        fh.write("#status\tmeaning\treads\n")
        for st in sorted(STATUS_NAMES):
            c = int((status == st).sum())
            if c:
                fh.write("status=%d\t%s\t%d\n" % (st, STATUS_NAMES[st], c))
    return folder


# ---- tags inside reads (`--demux_mid_tags`): the policy on top of ngsid_demux_scan (include/ngsid_demux.h, csrc/k_demux_scan.hip)
ST_MID_TAG = 5
MID_STATUS_NAME = "mid_tag"
MID_MODES = ("off", "discard", "split")
_TAG_COMPLEMENT = dict(zip("ACGTMKRYBVDHWSNX", "TGCAKMYRVBHDWSNX"))


def revcomp_tag(tag: str) -> str:
    """reverse complement over the tag alphabet: M-K, R-Y, B-V, D-H; W, S, N and X are their own complements"""
    return "".join(_TAG_COMPLEMENT[c] for c in reversed(tag))


def scan_patterns(sheet: Sheet):
    """the patterns of the scan: pattern t = tag t, pattern T + t = its reverse complement"""
    return list(sheet.tags) + [revcomp_tag(t) for t in sheet.tags]


def default_mid_max_ed(m: int) -> int:
    """the edit bound of an interior hit of a tag of m letters when --demux_mid_max_ed is not given.  The sweep of tools/demux_scan_sweep.py (profiles/demux.txt) settled
    1 at 13, 2 at 16 and 3 at 24 bases: per tag length the bound with the highest recall on planted concatemers among those at which no clean read had an interior hit.
    A length between two of the sweep takes the bound of the shorter one, a tag below 13 bases counts only as an exact copy."""
    return 3 if m >= 24 else 2 if m >= 16 else 1 if m >= 13 else 0


def interior_hits(hit_off, hits, pattern_len, lens, cut0, cut1, mid_max_ed):
    """the hits of Api.demux_scan that lie inside the read, away from its own end tags -> bool [H].

    A hit (pattern, end e, ed d) of a pattern of m letters in a read of L letters whose end tags were cut at cut0 / cut1 (assign() on the whole read; 0 where an end
    carries no tag) is interior iff d <= mid_max_ed, e - m - d + 1 >= cut0 and e < L - cut1.  mid_max_ed: one bound, or one per pattern."""
    hit_off = np.asarray(hit_off, dtype=np.int64); h = np.asarray(hits, dtype=np.int64).reshape(-1, 3)
    read = np.repeat(np.arange(len(hit_off) - 1), np.diff(hit_off))
    m = np.asarray(pattern_len, dtype=np.int64)[h[:, 0]]
    bound = np.broadcast_to(np.asarray(mid_max_ed, dtype=np.int64), (len(pattern_len),))[h[:, 0]] if np.ndim(mid_max_ed) else int(mid_max_ed)
    L = np.asarray(lens, dtype=np.int64)[read]; c0 = np.asarray(cut0, dtype=np.int64)[read]; c1 = np.asarray(cut1, dtype=np.int64)[read]
    e, d = h[:, 1], h[:, 2]
    return (d <= bound) & (e - m - d + 1 >= c0) & (e < L - c1)


def hit_cuts(hits, pattern_len, n_tags):
    """the cuts of interior hits [k, 3], sorted and distinct: a forward pattern (index < n_tags) starts an amplicon to its right - cut before it, at max(e - m - d + 1, 0),
    never behind its true start; a reverse-complement pattern ends an amplicon to its left - cut behind it, at e + 1"""
    h = np.asarray(hits, dtype=np.int64).reshape(-1, 3)
    m = np.asarray(pattern_len, dtype=np.int64)[h[:, 0]]
    return np.unique(np.where(h[:, 0] < int(n_tags), np.maximum(h[:, 1] - m - h[:, 2] + 1, 0), h[:, 1] + 1))


def pieces_of(cuts, L):
    """[(a, b)]: the non-empty intervals of [0, L) between the sorted distinct cuts"""
    edges = np.unique(np.concatenate(([0, int(L)], np.clip(np.asarray(cuts, dtype=np.int64), 0, int(L)))))
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def piece_name(header: str, k: int) -> str:
    """the header of piece k (1-based, left to right): /p<k> behind the first word"""
    for i, c in enumerate(header):
        if c in " \t":
            return "%s/p%d%s" % (header[:i], k, header[i:])
    return "%s/p%d" % (header, k)


def find_concatemers(api, work: ReadSet, sheet: Sheet, result, mid_max_ed=None):
    """scan the whole reads for the sheet's tags on both strands -> dict(reads [c] (indices of the reads with an interior hit, ascending), hits (list of [k, 3] arrays,
    the interior hits of each), pattern_len, patterns)"""
    pats = scan_patterns(sheet)
    plen = np.array([len(p) for p in pats], dtype=np.int64)
    bound = np.array([default_mid_max_ed(m) for m in plen], dtype=np.int64) if mid_max_ed is None else np.full(len(pats), int(mid_max_ed), dtype=np.int64)
    hit_off, hits = api.demux_scan(work, pats, max_ed=int(bound.max()), iupac=True)
    lens = np.diff(work.off.astype(np.int64))
    inner = interior_hits(hit_off, hits, plen, lens, result[3], result[4], bound)
    read = np.repeat(np.arange(work.n), np.diff(hit_off.astype(np.int64)))[inner]                  # ascending: the hits are grouped by read
    reads, first = np.unique(read, return_index=True)
    return dict(reads=reads, hits=np.split(hits[inner], first[1:]) if len(reads) else [], pattern_len=plen, patterns=pats)


def cut_pieces(names, rs: ReadSet, work: ReadSet, conc, n_tags):
    """the pieces of the reads conc["reads"] -> (piece names (list), piece read set with the original letters and qualities, the same with the searched letters,
    owner [p] = position of the piece's read in conc["reads"])"""
    off = rs.off.astype(np.int64)
    pn, seq, wseq, qual, owner = [], [], [], [], []
    for c, (r, h) in enumerate(zip(conc["reads"].tolist(), conc["hits"])):
        a0, L = int(off[r]), int(off[r + 1] - off[r])
        for k, (a, b) in enumerate(pieces_of(hit_cuts(h, conc["pattern_len"], n_tags), L), 1):
            pn.append(piece_name(names.get(r), k)); owner.append(c)
            seq.append(rs.seq[a0 + a:a0 + b]); wseq.append(work.seq[a0 + a:a0 + b])
            qual.append(rs.qual[a0 + a:a0 + b] if rs.qual is not None else np.full(b - a, ord("I"), dtype=np.uint8))
    poff = np.zeros(len(seq) + 1, dtype=np.uint64)
    if seq:
        poff[1:] = np.cumsum([len(s) for s in seq])
    cat = lambda xs: np.ascontiguousarray(np.concatenate(xs)) if xs else np.zeros(0, dtype=np.uint8)
    q = cat(qual)
    return pn, ReadSet(cat(seq), q, poff), ReadSet(cat(wseq), q, poff), np.array(owner, dtype=np.int64)


def write_outputs_mid(outfolder, sheet: Sheet, names, rs: ReadSet, hits, result, mode, conc, pieces=None, keep_tags=False):
    """the outputs of write_outputs with `--demux_mid_tags discard | split`: reads with an interior hit get status 5 (mid_tag).  discard: they go whole to
    demux_unassigned.fastq.  split: they are written nowhere; their pieces (pieces = (piece names, piece read set, hits and assign() result of the pieces, owner)) join
    their sample's file behind the whole reads, in input order, or demux_unassigned.fastq.  + demux_concatemers.tsv and the concatemer lines of demux_summary.tsv.
    -> (folder of the sample files, dict of the concatemer counts)"""
    sample, strand, status, cut0, cut1 = [np.array(x) for x in result]
    cr = conc["reads"]
    sample[cr] = -1; strand[cr] = -1; status[cr] = ST_MID_TAG
    folder = write_outputs(outfolder, sheet, names, rs, hits, (sample, strand, status, cut0, cut1), keep_tags=keep_tags)
    psample = np.zeros(0, dtype=np.int32); owner = np.zeros(0, dtype=np.int64)
    if mode == "split":
        pnames, prs, phits, presult, owner = pieces
        psample = presult[0]
        # the unassigned file holds the whole reads without a sample, the concatemers left out, then the pieces without one
        fastio.write_fastq(os.path.join(outfolder, "demux_unassigned.fastq"), np.flatnonzero((sample < 0) & (status != ST_MID_TAG)), names, rs)
        if len(pnames):
            pn = fastio.Names.from_list(pnames)
            out = prs if keep_tags else _trimmed(prs, presult[3], presult[4], psample >= 0)
            for s, name in enumerate(sheet.samples):
                idx = np.flatnonzero(psample == s)
                if len(idx):
                    fastio.write_fastq(os.path.join(folder, name + ".fastq"), idx, pn, out, append=True)
            fastio.write_fastq(os.path.join(outfolder, "demux_unassigned.fastq"), np.flatnonzero(psample < 0), pn, out, append=True)
    lens = np.diff(rs.off.astype(np.int64))
    T = len(sheet.tags)
    pat_name = lambda p: sheet.tags[p] if p < T else sheet.tags[p - T] + "/rc"
    first_word = lambda h: h.split()[0] if h.split() else h
    piece_at = np.searchsorted(owner, np.arange(len(cr) + 1))                                        # owner is ascending: the pieces of concatemer c are piece_at[c] .. piece_at[c + 1]
    one = many = 0
    with open(os.path.join(outfolder, "demux_concatemers.tsv"), "w") as fh:
        fh.write("#read\tlength\tpieces\thits\tpiece_samples\n")
        for c, (r, h) in enumerate(zip(cr.tolist(), conc["hits"])):
            mine = psample[piece_at[c]:piece_at[c + 1]]
            npieces = len(mine) if mode == "split" else len(pieces_of(hit_cuts(h, conc["pattern_len"], T), int(lens[r])))
            got = np.unique(mine[mine >= 0])
            one += len(got) == 1; many += len(got) > 1
            fh.write("%s\t%d\t%d\t%s\t%s\n" % (first_word(names.get(r)), int(lens[r]), npieces,
                                               ",".join("%s:%d:%d" % (pat_name(int(p)), int(e), int(d)) for p, e, d in h.tolist()),
                                               ",".join(sheet.samples[s] if s >= 0 else "-" for s in mine.tolist()) if mode == "split" else "-"))
    counts = dict(concatemers=int(len(cr)), pieces=int(len(psample)), pieces_assigned=int((psample >= 0).sum()), one_sample=int(one), several_samples=int(many))
    with open(os.path.join(outfolder, "demux_summary.tsv"), "a") as fh:
        if len(cr):
            fh.write("status=%d\t%s\t%d\n" % (ST_MID_TAG, MID_STATUS_NAME, len(cr)))
        fh.write("#mid_tags\tmeaning\tcount\n")
        fh.write("mid_tags=%s\treads_with_interior_hits\t%d\n" % (mode, counts["concatemers"]))
        fh.write("mid_tags=%s\tpieces_made\t%d\n" % (mode, counts["pieces"]))
        fh.write("mid_tags=%s\tpieces_assigned\t%d\n" % (mode, counts["pieces_assigned"]))
        fh.write("mid_tags=%s\tconcatemers_with_pieces_of_one_sample\t%d\n" % (mode, counts["one_sample"]))
        fh.write("mid_tags=%s\tconcatemers_with_pieces_of_several_samples\t%d\n" % (mode, counts["several_samples"]))
    return folder, counts


def run(args, api):
    """the `--demux_sheet` step of the command line: ingest the pooled file once, locate, assign, write -> (folder of the sample files, summary dict)"""
    from time import time
    T = {}
    t0 = time()
    sheet = read_sheet(args.demux_sheet)
    names, rs, _ = fastio.read_fastq(args.fastq)
    T["read_fastq"] = time() - t0; t0 = time()
    work = rs
    if rs.n and fastio.count_foreign_bases(rs.seq):
        seq = rs.seq.copy()
        changed = fastio.normalize_bases(seq)
        logging.warning("%d bases outside A/C/G/T/N are searched as upper case / N; the output files keep the original letters", changed)
        work = ReadSet(seq, None, rs.off)
    hits = api.demux_locate(work, sheet.tags, window=args.demux_window, max_ed=args.demux_max_ed, iupac=True) if rs.n else np.zeros((0, 2, 5), np.int32)
    T["demux_locate"] = time() - t0; t0 = time()
    result = assign(hits, sheet, args.demux_min_margin, lens=np.diff(rs.off.astype(np.int64)))
    keep_tags = bool(getattr(args, "demux_keep_tags", False))
    mode = getattr(args, "demux_mid_tags", None) or "off"
    if mode == "off":
        folder = write_outputs(args.outfolder, sheet, names, rs, hits, result, keep_tags=keep_tags)
        T["demux_write"] = time() - t0
        n_assigned = int((result[0] >= 0).sum())
        logging.info("Demultiplexed %d reads: %d assigned to %d of %d samples" % (rs.n, n_assigned, len(np.unique(result[0][result[0] >= 0])), len(sheet.samples)))
        return folder, dict(reads=int(rs.n), assigned=n_assigned, timings=T)
    # ---- tags inside the reads: scan, then discard the reads that carry one or split them and send the pieces through locate + assign once more (pieces are not scanned again)
    empty = dict(reads=np.zeros(0, dtype=np.int64), hits=[], pattern_len=np.array([len(p) for p in scan_patterns(sheet)], dtype=np.int64), patterns=scan_patterns(sheet))
    conc = find_concatemers(api, work, sheet, result, getattr(args, "demux_mid_max_ed", None)) if rs.n else empty
    T["demux_scan"] = time() - t0; t0 = time()
    pieces = None
    if mode == "split":
        pnames, prs, pwork, owner = cut_pieces(names, rs, work, conc, len(sheet.tags))
        phits = api.demux_locate(pwork, sheet.tags, window=args.demux_window, max_ed=args.demux_max_ed, iupac=True) if prs.n else np.zeros((0, 2, 5), np.int32)
        pieces = (pnames, prs, phits, assign(phits, sheet, args.demux_min_margin, lens=np.diff(prs.off.astype(np.int64))), owner)
        T["demux_locate_pieces"] = time() - t0; t0 = time()
    folder, counts = write_outputs_mid(args.outfolder, sheet, names, rs, hits, result, mode, conc, pieces, keep_tags=keep_tags)
    T["demux_write"] = time() - t0
    whole = np.array(result[0]); whole[conc["reads"]] = -1
    n_assigned = int((whole >= 0).sum())
    logging.info("Demultiplexed %d reads: %d assigned to %d of %d samples; %d reads with a tag inside (%s): %d pieces, %d assigned"
                 % (rs.n, n_assigned, len(np.unique(whole[whole >= 0])), len(sheet.samples), counts["concatemers"], mode, counts["pieces"], counts["pieces_assigned"]))
    return folder, dict(reads=int(rs.n), assigned=n_assigned, mid_tags=counts, timings=T)
