"""Read-to-consensus alignments as SAM (extension; include/ngsid_cigar.h, csrc/k_cigar.hip, ngsid_host_write_sam in csrc/host_io.hip).

Api.read_cigars returns the alignment of every listed read to the centre of its group as integers (span, nm, run-length-encoded BAM ops) and the library's record
writer formats the file; this module holds the policy and no arithmetic on alignments:
  header        @HD, one @SQ per target, @PG
  lists         which reads are listed under which consensus: by default the pooled lists the polisher takes (as for --consensus_support); with a recruit result every
                ASSIGNED read under its recruited consensus, the ambiguous ones as unmapped records beside their nearest consensus, the unassigned ones nowhere
                (the `sam` sub-command, whose one file holds every target, lists them as unmapped records too)
  align         ONE Api.read_cigars call for all consensuses of all samples, cut back per consensus
  capacity      the count call, then the fill call (cap=None).  The count call repeats the store pass; a caller who knows a bound passes cap and saves it
                (2 * nm + 3 ops bound one read, but nm is not known beforehand).  No estimate-and-retry here: a retry would repeat the pass as well, and a wrong guess
                costs more than the count call (profiles/cigar.txt)
and cigar_strings / parse_sam for small sets, tests and tools."""
from __future__ import annotations
import os
import numpy as np
from ._capi import ReadSet, CIGAR_OPS

PROGRAM = "ngspeciesid_amd"
READ_OPS, REF_OPS = frozenset("M=XIS"), frozenset("M=XD")          # the ops that consume the read / the target


def header(tnames, tlens, command_line=None) -> str:
    """the header text: @HD, one @SQ per target, @PG"""
    lines = ["@HD\tVN:1.6\tSO:unknown"] + ["@SQ\tSN:%s\tLN:%d" % (n, int(l)) for n, l in zip(tnames, tlens)]
    lines.append("@PG\tID:%s\tPN:%s" % (PROGRAM, PROGRAM) + ("\tCL:%s" % command_line.replace("\t", " ") if command_line else ""))
    return "\n".join(lines) + "\n"


def cigar_strings(op_off, ops):
    """the CIGAR text of every listed read of an Api.read_cigars result ('*' for a read without ops) - for small sets and tests; files are formatted by the library"""
    op_off = np.asarray(op_off).astype(np.int64); ops = np.asarray(ops).astype(np.int64)
    out = []
    for a, b in zip(op_off[:-1].tolist(), op_off[1:].tolist()):
        out.append("".join("%d%s" % (v >> 4, CIGAR_OPS[v & 15]) for v in ops[a:b].tolist()) if b > a else "*")
    return out


def cigar_ops(text):
    """'3S10=1X' -> [(3, 'S'), (10, '='), (1, 'X')]; '*' -> []"""
    out, n = [], 0
    if text == "*":
        return out
    for ch in text:
        if ch.isdigit(): n = n * 10 + ord(ch) - 48
        else: out.append((n, ch)); n = 0
    return out


def parse_sam(path) -> dict:
    """-> dict(header = the header lines, targets = [(name, length)], and one array per field of the records: qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen,
    seq, qual (object or int64 arrays), nm (int64, -1 without the tag))"""
    head, rows = [], []
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith("@"): head.append(line)
            elif line: rows.append(line.split("\t"))
    targets = []
    for h in head:
        if h.startswith("@SQ"):
            tags = dict(t.split(":", 1) for t in h.split("\t")[1:])
            targets.append((tags["SN"], int(tags["LN"])))
    if any(len(r) < 11 for r in rows):
        raise ValueError("%s: a record with fewer than 11 fields" % path)
    col = lambda i, t: np.array([r[i] for r in rows], dtype=object) if t is str else np.array([int(r[i]) for r in rows], dtype=np.int64)
    nm = np.array([next((int(t[5:]) for t in r[11:] if t.startswith("NM:i:")), -1) for r in rows], dtype=np.int64)
    return dict(header=head, targets=targets, qname=col(0, str), flag=col(1, int), rname=col(2, str), pos=col(3, int), mapq=col(4, int), cigar=col(5, str),
                rnext=col(6, str), pnext=col(7, int), tlen=col(8, int), seq=col(9, str), qual=col(10, str), nm=nm)


def recruited_lists(hits, status, n_centres):
    """the lists of a recruit result (recruit.run: hits with centre numbers, status) -> (lists[c] = the reads ASSIGNED to centre c, near[c] = the ambiguous reads whose
    nearest centre is c, unassigned = the reads without a centre), read numbers ascending"""
    from . import recruit
    h = np.asarray(hits).reshape(-1, 6); st = np.asarray(status)
    lists = [np.nonzero((st == recruit.ASSIGNED) & (h[:, 0] == c))[0].astype(np.uint32) for c in range(int(n_centres))]
    near = [np.nonzero((st == recruit.AMBIGUOUS) & (h[:, 0] == c))[0].astype(np.uint32) for c in range(int(n_centres))]
    return lists, near, np.nonzero(st == recruit.UNASSIGNED)[0].astype(np.uint32)


def align(api, rs, seqs, lists, k=13, w=20, clip=False, merge_m=False, cap=None):
    """Api.read_cigars of the sequences seqs over their read lists, ONE call -> one dict(reads, strand, aln, op_off, ops) per sequence (op_off starts at 0)"""
    if not seqs:
        return []
    go = np.concatenate(([0], np.cumsum([len(l) for l in lists]))).astype(np.uint64)
    ro = np.concatenate(lists).astype(np.uint32) if len(lists) else np.zeros(0, np.uint32)
    aln, op_off, ops, strand = api.read_cigars(ReadSet.from_strings(list(seqs)), rs, go, read_order=ro, k=k, w=w, clip=clip, merge_m=merge_m, cap=cap)
    out = []
    for c in range(len(seqs)):
        a, b = int(go[c]), int(go[c + 1]); oa, ob = int(op_off[a]), int(op_off[b])
        out.append(dict(reads=np.asarray(lists[c]), strand=strand[a:b], aln=aln[a:b], op_off=op_off[a:b + 1] - op_off[a], ops=ops[oa:ob]))
    return out


def write(path, names, rs, tnames, tlens, parts, extra_unmapped=None, suffixes=None, flip=None, command_line=None, jobs=None):
    """one SAM file: parts = [(target number, entry of align())], in that order, then the reads extra_unmapped as unmapped records.  rs: the HOST read set the records take
    SEQ and QUAL from; flip[r] != 0: read r of rs is the reverse complement of the read that was aligned (--strand_aware)."""
    from . import fastio
    extra = np.zeros(0, np.uint32) if extra_unmapped is None else np.asarray(extra_unmapped, dtype=np.uint32)
    idx = np.concatenate([np.asarray(e["reads"], dtype=np.uint32) for _, e in parts] + [extra]) if parts or len(extra) else np.zeros(0, np.uint32)
    strand = np.concatenate([e["strand"] for _, e in parts] + [np.full(len(extra), -1, np.int8)]).astype(np.int8) if len(idx) else np.zeros(0, np.int8)
    if flip is not None and len(idx):
        f = np.asarray(flip)[idx].astype(np.int8)
        strand = np.where(strand >= 0, strand ^ f, strand).astype(np.int8)
    target = np.concatenate([np.full(len(e["reads"]), t, np.int32) for t, e in parts] + [np.full(len(extra), -1, np.int32)]) if len(idx) else np.zeros(0, np.int32)
    aln = np.concatenate([e["aln"].reshape(-1, 5) for _, e in parts] + [np.full((len(extra), 5), -1, np.int32)]) if len(idx) else np.zeros((0, 5), np.int32)
    counts = np.concatenate([np.diff(e["op_off"].astype(np.int64)) for _, e in parts] + [np.zeros(len(extra), np.int64)]) if len(idx) else np.zeros(0, np.int64)
    op_off = np.zeros(len(idx) + 1, dtype=np.uint64); op_off[1:] = np.cumsum(counts)
    ops = np.concatenate([e["ops"] for _, e in parts]) if parts else np.zeros(0, np.uint32)
    fastio.write_sam(path, header(tnames, tlens, command_line), idx, names, rs, strand, target, list(tnames), aln, op_off, ops, suffixes=suffixes, jobs=jobs)
    return int(((target >= 0) & (strand >= 0) & (aln[:, 0] >= 0)).sum()), len(idx)          # (mapped records, records)


# ---- the command line
def add_flags(p):
    p.add_argument('--write_sam', action='store_true', help='extension: the alignment of every read to its consensus as SAM (CIGAR with = and X, NM tag). Writes racon_cl_id_*/reads_to_consensus.sam; without --racon, consensus_reference_{id}.sam. The reads listed are the pooled reads the polisher takes; with --recruit, every read under the consensus it was recruited to')
    p.add_argument('--sam_merge_m', action='store_true', help='extension: --write_sam writes M instead of = and X')


def check_args(args):
    if getattr(args, "sam_merge_m", False) and not getattr(args, "write_sam", False) and getattr(args, "which", "main") != "sam":
        return "--sam_merge_m is an option of --write_sam."
    return None


def sam_fastq(args, api=None):
    """the `sam` sub-command: the reads of --fastq recruited to the sequences of --fasta (recruit.py's defaults), every assigned read aligned to its sequence -> ONE SAM
    with every sequence of the FASTA as a target; ambiguous and unassigned reads (and assigned reads the aligner finds no strand for) are unmapped records"""
    from . import runtime, fastio, recruit
    from .help_functions import readfq
    api = api or runtime.get_api()
    with open(args.fasta) as fh:
        cons = [(name.split()[0] if name.split() else "", sq[0].upper()) for name, sq in readfq(fh)]
    names, rs, _ = fastio.read_fastq(args.fastq)
    seq = rs.seq.copy(); fastio.normalize_bases(seq)
    rs = ReadSet(seq, rs.qual, rs.off)
    tnames = [c[0] for c in cons]; seqs = [c[1] for c in cons]
    res = recruit.run(api, rs, [0, rs.n], [seqs], min_identity=getattr(args, "recruit_min_identity", None), q=getattr(args, "quality_threshold", 7.0),
                      min_margin=getattr(args, "recruit_min_margin", 1), both_strands=not getattr(args, "recruit_one_strand", False))[0]
    lists, near, unassigned = recruited_lists(res["hits"], res["status"], len(seqs))
    parts = align(api, rs, seqs, lists, k=getattr(args, "k", 13), w=getattr(args, "w", 20), merge_m=getattr(args, "sam_merge_m", False))
    rest = np.sort(np.concatenate(near + [unassigned])) if len(seqs) else np.arange(rs.n, dtype=np.uint32)
    mapped, n = write(args.outfile, names, rs, tnames, [len(q) for q in seqs], list(enumerate(parts)), extra_unmapped=rest)
    return dict(mapped=mapped, records=n, recruit=res)
