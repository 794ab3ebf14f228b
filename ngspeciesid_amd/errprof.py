"""Read error profile and quality calibration (extension; include/ngsid_errprof.h, csrc/k_errprof.hip).

Api.error_profile returns integer tables per consensus and strand: which centre letter became what, how long insertions and deletions are, how errors depend on the
homopolymer run a base sits in, and how often a read base of reported quality q sat in a match, a mismatch or an insertion column.  This module holds the policy and
no device work, in numpy: which reads are listed under which consensus, what is called a rate, the pseudo-count of the calibration, and the files.

WHAT THE TABLES CANNOT SEE.  The centre is made of the same reads it is compared with.  An error the majority of a cluster shares (a systematic homopolymer
undercall, say) is in the consensus and therefore invisible here; a true minority variant in a cluster (a second haplotype, a paralogue) counts as read error.  Split
such clusters first (--split_haplotypes) when the figures matter.  The alignment is a minimum-edit one: errors that cancel are not seen, and an indel inside a
homopolymer is placed where the aligner's tie-break puts it (profiles/errprof.txt records what that does to a known generator).

  rates         per strand and both: substitutions, inserted bases and deleted bases per aligned centre base of ACGT, and their sum
  spectrum      the 4 x 4 shares of the substitutions (centre letter x read letter)
  indel_lengths the run-length histograms of insertions and deletions
  hp_table      per centre run length 1 .. 8+: mismatch, deletion and insertion-behind rates
  calibration   per reported quality q: bases, errors (mismatch + insertion) and the empirical Phred of (errors + 1) / (bases + 2)
  summary       one read error rate and its Phred equivalent beside the mean reported error of the same bases
  profile       ONE Api.error_profile call for all consensuses of all samples
  write / read_table, write_calibration / read_calibration: error_profile.tsv and quality_calibration.tsv"""
from __future__ import annotations
import os
import numpy as np
from ._capi import (ReadSet, ERRPROF_NCOUNT, ERRPROF_NQ, ERRPROF_PAIR, ERRPROF_INS_LETTER, ERRPROF_CEN_OTHER, ERRPROF_READS, ERRPROF_INS_LEN, ERRPROF_DEL_LEN,
                    ERRPROF_HPCTX)

LETTERS = ("A", "C", "G", "T")
MIN_OBS = 100                    # calibration: a quality bin with fewer bases is not reported (the pseudo-count alone would speak)
# the tables of counts as (name, first entry, rows, columns): the long format of error_profile.tsv and its inverse
TABLES = (("PAIR", ERRPROF_PAIR, LETTERS, LETTERS + ("other", "del")),
          ("INS_LETTER", ERRPROF_INS_LETTER, ("-",), LETTERS + ("other",)),
          ("CEN_OTHER", ERRPROF_CEN_OTHER, ("-",), ("-",)),
          ("READS", ERRPROF_READS, ("-",), ("-",)),
          ("INS_LEN", ERRPROF_INS_LEN, ("-",), tuple(str(l) for l in range(1, 16)) + ("16+",)),
          ("DEL_LEN", ERRPROF_DEL_LEN, ("-",), tuple(str(l) for l in range(1, 16)) + ("16+",)),
          ("HPCTX", ERRPROF_HPCTX, tuple(str(r) for r in range(1, 8)) + ("8+",), ("match", "sub", "del", "ins_behind")))
STRANDS = ("0", "1", "both")
RATE_NAMES = ("aligned", "substitution", "insertion", "deletion", "total")
TABLE_HEADER = ("cluster_id", "strand", "table", "row", "col", "count")
RATE_HEADER = ("cluster_id", "strand", "rate", "value")
CALIBRATION_HEADER = ("q", "n_match", "n_sub", "n_ins", "empirical_q")


def _by_strand(counts):
    """counts [..., 2, 96] -> float [3, 96]: strand 0, strand 1, both, summed over everything in front"""
    c = np.asarray(counts, dtype=np.float64).reshape(-1, 2, ERRPROF_NCOUNT).sum(axis=0)
    return np.vstack((c, c.sum(axis=0, keepdims=True)))


def _div(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.divide(a, b, out=np.zeros(np.broadcast(a, b).shape), where=b > 0)


def rates(counts) -> dict:
    """-> {"0" | "1" | "both": dict(aligned, substitution, insertion, deletion, total)}: aligned = the '=', 'X' and 'D' columns of centre bases of ACGT; the rates are
    mismatch columns, inserted BASES and deleted bases per aligned centre base (0 where nothing aligned), total their sum"""
    out = {}
    for name, c in zip(STRANDS, _by_strand(counts)):
        pair = c[ERRPROF_PAIR:ERRPROF_PAIR + 24].reshape(4, 6)
        aligned = pair.sum(); dele = pair[:, 5].sum(); sub = aligned - dele - np.trace(pair[:, :4]); ins = c[ERRPROF_INS_LETTER:ERRPROF_INS_LETTER + 5].sum()
        r = dict(aligned=float(aligned), substitution=float(_div(sub, aligned)), insertion=float(_div(ins, aligned)), deletion=float(_div(dele, aligned)))
        r["total"] = r["substitution"] + r["insertion"] + r["deletion"]
        out[name] = r
    return out


def spectrum(counts):
    """-> [4, 4] float: share of every centre letter -> read letter substitution among the substitutions between letters of ACGT, both strands (zeros without one)"""
    pair = _by_strand(counts)[2][ERRPROF_PAIR:ERRPROF_PAIR + 24].reshape(4, 6)[:, :4].copy()
    np.fill_diagonal(pair, 0.0)
    return _div(pair, pair.sum())


def indel_lengths(counts) -> dict:
    """-> dict(ins [16], dele [16]: runs by length 1 .. 15, 16+, both strands; ins_share, del_share: the same as shares of their kind)"""
    c = _by_strand(counts)[2]
    ins = c[ERRPROF_INS_LEN:ERRPROF_INS_LEN + 16]; dele = c[ERRPROF_DEL_LEN:ERRPROF_DEL_LEN + 16]
    return dict(ins=ins.astype(np.uint64), dele=dele.astype(np.uint64), ins_share=_div(ins, ins.sum()), del_share=_div(dele, dele.sum()))


def hp_table(counts) -> dict:
    """-> dict(n [8], sub [8], dele [8], ins_behind [8]): per length 1 .. 8+ of the centre run a base sits in, the aligned bases and the share of them that are a
    mismatch, deleted, or directly followed by an insertion; both strands"""
    h = _by_strand(counts)[2][ERRPROF_HPCTX:ERRPROF_HPCTX + 32].reshape(8, 4)
    n = h[:, :3].sum(axis=1)
    return dict(n=n.astype(np.uint64), sub=_div(h[:, 1], n), dele=_div(h[:, 2], n), ins_behind=_div(h[:, 3], n))


def calibration(qtab, min_obs=MIN_OBS) -> dict:
    """qtab [..., 94, 3] -> dict(q, n_match, n_sub, n_ins, empirical_q): one row per reported quality with at least min_obs read bases (match + mismatch + inserted);
    empirical_q = -10 log10((n_sub + n_ins + 1) / (n + 2)) - the pseudo-count keeps a bin without an error finite.  Deleted bases have no quality and are not here."""
    t = np.asarray(qtab, dtype=np.float64).reshape(-1, ERRPROF_NQ, 3).sum(axis=0)
    n = t.sum(axis=1); keep = (n >= max(float(min_obs), 1.0))
    q = np.nonzero(keep)[0]
    emp = -10.0 * np.log10((t[q, 1] + t[q, 2] + 1.0) / (n[q] + 2.0))
    return dict(q=q.astype(np.int64), n_match=t[q, 0].astype(np.uint64), n_sub=t[q, 1].astype(np.uint64), n_ins=t[q, 2].astype(np.uint64), empirical_q=emp)


def summary(counts, qtab=None) -> dict:
    """-> dict(bases, errors, error_rate, phred, reported_error, reported_phred): the read bases of the counted columns, those in a mismatch or an insertion column,
    their share and its Phred equivalent; with qtab the mean error probability the same bases REPORT (10^(-q / 10)) and its Phred (None without qualities)"""
    c = _by_strand(counts)[2]
    pair = c[ERRPROF_PAIR:ERRPROF_PAIR + 24].reshape(4, 6)
    bases = pair[:, :5].sum() + c[ERRPROF_INS_LETTER:ERRPROF_INS_LETTER + 5].sum()
    errors = bases - np.trace(pair[:, :4])
    rate = float(_div(errors, bases))
    res = dict(bases=int(bases), errors=int(errors), error_rate=rate, phred=float(-10.0 * np.log10(rate)) if rate > 0 else None, reported_error=None, reported_phred=None)
    if qtab is not None:
        n = np.asarray(qtab, dtype=np.float64).reshape(-1, ERRPROF_NQ, 3).sum(axis=(0, 2))
        if n.sum() > 0:
            rep = float((n * 10.0 ** (-np.arange(ERRPROF_NQ) / 10.0)).sum() / n.sum())
            res.update(reported_error=rep, reported_phred=float(-10.0 * np.log10(rep)))
    return res


def profile(api, rs, seqs, lists, k=13, w=20, clip=False, qualities=True):
    """Api.error_profile of the sequences seqs over their read lists, ONE call -> one dict(counts [2, 96], qtab [2, 94, 3] or None, n_listed, n_stranded) per sequence"""
    if not seqs:
        return []
    go = np.concatenate(([0], np.cumsum([len(l) for l in lists]))).astype(np.uint64)
    ro = np.concatenate(lists).astype(np.uint32) if len(lists) else np.zeros(0, np.uint32)
    counts, qtab, strand = api.error_profile(ReadSet.from_strings(list(seqs)), rs, go, read_order=ro, k=k, w=w, clip=clip, qualities=qualities)
    return [dict(counts=counts[c], qtab=None if qtab is None else qtab[c], n_listed=int(go[c + 1] - go[c]), n_stranded=int((strand[int(go[c]):int(go[c + 1])] >= 0).sum()))
            for c in range(len(seqs))]


# ---- files
def table_rows(cluster_id, counts):
    """the long rows (cluster_id, strand, table, row, col, count) of one [2, 96] table: every non-zero entry, and READS always"""
    c = np.asarray(counts).reshape(2, ERRPROF_NCOUNT)
    rows = []
    for s in (0, 1):
        for name, at, rws, cols in TABLES:
            for i, r in enumerate(rws):
                for j, cl in enumerate(cols):
                    v = int(c[s, at + i * len(cols) + j])
                    if v or name == "READS": rows.append((str(cluster_id), str(s), name, r, cl, v))
    return rows


def rate_rows(cluster_id, counts):
    r = rates(counts)
    return [(str(cluster_id), s, name, repr(float(r[s][name]))) for s in STRANDS for name in RATE_NAMES]


def write(path, entries, sample=None, header=True, mode="w"):
    """error_profile.tsv: entries = [(cluster_id, counts [2, 96])].  A block of counts in long format, a blank line, a block of rates; sample: a first column"""
    pre = () if sample is None else (str(sample),)
    with open(path, mode) as f:
        if header: f.write("\t".join((("sample",) if sample is not None else ()) + TABLE_HEADER) + "\n")
        for cid, c in entries:
            for row in table_rows(cid, c): f.write("\t".join(pre + tuple(str(x) for x in row)) + "\n")
        f.write("\n")
        if header: f.write("\t".join((("sample",) if sample is not None else ()) + RATE_HEADER) + "\n")
        for cid, c in entries:
            for row in rate_rows(cid, c): f.write("\t".join(pre + row) + "\n")


def read_table(path) -> dict:
    """the inverse of write for a file without a sample column -> dict(counts = {cluster_id: [2, 96] uint64}, rates = {cluster_id: {strand: {rate: value}}})"""
    where = {name: (at, rws, cols) for name, at, rws, cols in TABLES}
    counts, rts = {}, {}
    with open(path) as f:
        for line in f:
            p = line.rstrip("\n").split("\t")
            if len(p) == len(TABLE_HEADER) and tuple(p) != TABLE_HEADER:
                at, rws, cols = where[p[2]]
                counts.setdefault(p[0], np.zeros((2, ERRPROF_NCOUNT), dtype=np.uint64))[int(p[1]), at + rws.index(p[3]) * len(cols) + cols.index(p[4])] = int(p[5])
            elif len(p) == len(RATE_HEADER) and tuple(p) != RATE_HEADER:
                rts.setdefault(p[0], {}).setdefault(p[1], {})[p[2]] = float(p[3])
    return dict(counts=counts, rates=rts)


def write_calibration(path, qtab, min_obs=MIN_OBS, sample=None, header=True, mode="w"):
    """quality_calibration.tsv: q, n_match, n_sub, n_ins, empirical_q of calibration(qtab, min_obs)"""
    cal = calibration(qtab, min_obs)
    pre = () if sample is None else (str(sample),)
    with open(path, mode) as f:
        if header: f.write("\t".join((("sample",) if sample is not None else ()) + CALIBRATION_HEADER) + "\n")
        for i in range(len(cal["q"])):
            f.write("\t".join(pre + (str(int(cal["q"][i])), str(int(cal["n_match"][i])), str(int(cal["n_sub"][i])), str(int(cal["n_ins"][i])), "%.3f" % cal["empirical_q"][i])) + "\n")


def read_calibration(path) -> dict:
    rows = [l.rstrip("\n").split("\t") for l in open(path)][1:]
    return dict(q=np.array([int(r[0]) for r in rows], dtype=np.int64), n_match=np.array([int(r[1]) for r in rows], dtype=np.uint64), n_sub=np.array([int(r[2]) for r in rows], dtype=np.uint64),
                n_ins=np.array([int(r[3]) for r in rows], dtype=np.uint64), empirical_q=np.array([float(r[4]) for r in rows]))


def write_sample(folder, ids, parts, min_obs=MIN_OBS):
    """the two files of one sample: parts = profile()'s entries of its consensuses ids"""
    write(os.path.join(folder, "error_profile.tsv"), [(i, p["counts"]) for i, p in zip(ids, parts)])
    write_calibration(os.path.join(folder, "quality_calibration.tsv"), _qsum(parts), min_obs)


def append_all(outfolder, sample, ids, parts, first, min_obs=MIN_OBS):
    """error_profile_all.tsv and quality_calibration_all.tsv of a multi-sample run: the sample's own files with the sample in front"""
    write(os.path.join(outfolder, "error_profile_all.tsv"), [(i, p["counts"]) for i, p in zip(ids, parts)], sample=sample, header=first, mode="w" if first else "a")
    write_calibration(os.path.join(outfolder, "quality_calibration_all.tsv"), _qsum(parts), min_obs, sample=sample, header=first, mode="w" if first else "a")


def _qsum(parts):
    q = [p["qtab"] for p in parts if p["qtab"] is not None]
    return np.sum(q, axis=0) if q else np.zeros((2, ERRPROF_NQ, 3), dtype=np.uint64)


# ---- the command line
def add_flags(p):
    p.add_argument('--error_profile', action='store_true', help='extension: the error profile of the reads against their consensus and the calibration of their qualities. Writes error_profile.tsv (cluster_id strand table row col count, then the rates) and quality_calibration.tsv (q n_match n_sub n_ins empirical_q). The reads listed are the pooled reads the polisher takes; with --recruit, every read under the consensus it was recruited to. The consensus is made of the same reads: a shared error is invisible, a minority variant counts as error (see --split_haplotypes)')


def errprof_fastq(args, api=None):
    """the `errprof` sub-command: the reads of --fastq recruited to the sequences of --fasta (recruit.py's defaults, as the `sam` sub-command), every assigned read
    profiled against its sequence -> error_profile.tsv, quality_calibration.tsv in --outfolder"""
    from . import runtime, fastio, recruit, sam
    from .help_functions import readfq
    api = api or runtime.get_api()
    with open(args.fasta) as fh:
        cons = [(name.split()[0] if name.split() else "", sq[0].upper()) for name, sq in readfq(fh)]
    names, rs, _ = fastio.read_fastq(args.fastq)
    seq = rs.seq.copy(); fastio.normalize_bases(seq)
    rs = ReadSet(seq, rs.qual, rs.off)
    ids = [c[0] for c in cons]; seqs = [c[1] for c in cons]
    res = recruit.run(api, rs, [0, rs.n], [seqs], min_identity=getattr(args, "recruit_min_identity", None), q=getattr(args, "quality_threshold", 7.0),
                      min_margin=getattr(args, "recruit_min_margin", 1), both_strands=not getattr(args, "recruit_one_strand", False))[0]
    lists, _, _ = sam.recruited_lists(res["hits"], res["status"], len(seqs))
    parts = profile(api, rs, seqs, lists, k=getattr(args, "k", 13), w=getattr(args, "w", 20))
    os.makedirs(args.outfolder, exist_ok=True)
    write_sample(args.outfolder, ids, parts)
    return dict(ids=ids, parts=parts, lists=lists, recruit=res)
