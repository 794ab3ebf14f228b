"""Demultiplexing of a pooled run (extension; `--demux_sheet`): the policy on top of ngsid_demux_locate (include/ngsid_demux.h, csrc/k_demux.hip).

The library locates every sample tag in both end windows of every read and returns integers.  Which read goes to which sample - the sheet, the margin
between the best and the second-best tag, the strand rule, the cuts - is decided here, and the files a demultiplexer leaves are written here:
<outfolder>/demux/<sample>.fastq, <outfolder>/demux_unassigned.fastq, <outfolder>/demux_summary.tsv.
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
    folder = write_outputs(args.outfolder, sheet, names, rs, hits, result, keep_tags=bool(getattr(args, "demux_keep_tags", False)))
    T["demux_write"] = time() - t0
    n_assigned = int((result[0] >= 0).sum())
    logging.info("Demultiplexed %d reads: %d assigned to %d of %d samples" % (rs.n, n_assigned, len(np.unique(result[0][result[0] >= 0])), len(sheet.samples)))
    return folder, dict(reads=int(rs.n), assigned=n_assigned, timings=T)
