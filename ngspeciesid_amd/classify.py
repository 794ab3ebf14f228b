"""Naming consensuses against a reference library (extension; `--reference_db`, sub-command `classify`): the policy on top of ngsid_refdb_build /
ngsid_classify_search (include/ngsid_classify.h, csrc/k_classify.hip).

The library counts the minimizers every consensus shares with every reference, on both strands, and returns the best top_k references per consensus as integers.
What happens to these candidates - the verification alignment (one Api.sg_align_cigar_batch call over all pairs, with the reference tool's own parasail
parameters), identity and coverage from its columns, the order of the hits, the thresholds that call one - is decided here, and the table is written here.

The default thresholds (identity 0.9, query coverage 0.8, 8 candidates, 3 shared minimizers, 5 rows reported) are policy choices, not measurements.
"""
from __future__ import annotations
import re
import numpy as np
from . import fastio
from ._capi import ReadSet, CLASSIFY_MAX_TOPK, CLASSIFY_MAX_K
from .hostutil import subset_reads

ALN_MATCH, ALN_MISMATCH, ALN_OPEN, ALN_EXT = 2, -2, 3, 1          # parasail_alignment of the reference tool (cluster.py:130-136)
DEFAULTS = dict(k=13, w=20, top_k=8, min_shared=3, min_identity=0.9, min_query_cov=0.8, report=5)
COLUMNS = ("consensus_id", "n_reads", "rank", "reference", "strand", "shared", "identity", "aln_cols", "n_match", "q_cov", "r_cov", "called", "header")
_FLOATS = ("identity", "q_cov", "r_cov")

_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


class Library:
    """names [R] (header up to the first blank), headers [R] (whole header lines without '>'), rs (host ReadSet of the normalised sequences), changed (letters normalised)"""

    def __init__(self, names, headers, rs, changed):
        self.names, self.headers, self.rs, self.changed = list(names), list(headers), rs, int(changed)

    def __len__(self):
        return len(self.names)


def read_reference_fasta(path, unique_names=True) -> Library:
    """multi-line FASTA -> Library.  Sequences are normalised like reads (upper case, anything outside ACGTN -> N; the count is Library.changed).  An empty record and,
    with unique_names, a name that occurs twice are ValueErrors that carry the record number (1-based)."""
    names, headers, parts, seen = [], [], [], {}
    cur = None
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if cur is not None:
                    parts.append("".join(cur))
                header = line[1:]
                name = header.split(None, 1)[0] if header.split() else ""
                names.append(name); headers.append(header); cur = []
            elif line.strip():
                if cur is None:
                    raise ValueError("%s: sequence data before the first '>' header" % path)
                cur.append(line.strip())
    if cur is not None:
        parts.append("".join(cur))
    for i, (name, seq) in enumerate(zip(names, parts), 1):
        if not name:
            raise ValueError("%s, record %d: empty header" % (path, i))
        if not seq:
            raise ValueError("%s, record %d (%s): empty record" % (path, i, name))
        if unique_names and name in seen:
            raise ValueError("%s, record %d: name %r was used by record %d already" % (path, i, name, seen[name]))
        seen.setdefault(name, i)
    rs = ReadSet.from_strings(parts)
    changed = fastio.normalize_bases(rs.seq) if len(rs.seq) else 0
    return Library(names, headers, rs, changed)


def identity_from_columns(cols: str):
    """one '=XID' column string of Api.sg_align_cigar_batch (I = query only, D = reference only) -> dict(aln_cols, n_match, identity, q_cov, r_cov).
    The leading and the trailing run of I / D are the free end gaps: they are stripped; aln_cols = length of the rest, n_match = its '=' columns,
    identity = n_match / aln_cols (float64; 0.0 when nothing remains), q_cov / r_cov = share of the query's / the reference's bases inside the rest."""
    core = cols.strip("ID")
    n = len(core)
    n_match = core.count("=")
    qlen = len(cols) - cols.count("D"); rlen = len(cols) - cols.count("I")
    q_in = n - core.count("D"); r_in = n - core.count("I")
    return dict(aln_cols=n, n_match=n_match, identity=(float(np.float64(n_match) / np.float64(n)) if n else 0.0),
                q_cov=(float(np.float64(q_in) / np.float64(qlen)) if qlen and n else 0.0), r_cov=(float(np.float64(r_in) / np.float64(rlen)) if rlen and n else 0.0))


def _as_readset(x):
    return x if isinstance(x, ReadSet) else ReadSet.from_strings(list(x))


def both_strands(queries: ReadSet) -> ReadSet:
    """sequence 2 q = query q, 2 q + 1 = its reverse complement (N stays N)"""
    off = queries.off.astype(np.int64); lens = np.diff(off)
    noff = np.zeros(2 * len(lens) + 1, dtype=np.uint64); noff[1:] = np.cumsum(np.repeat(lens, 2))
    seq = np.empty(int(noff[-1]), dtype=np.uint8)
    for q in range(len(lens)):
        s = queries.seq[off[q]:off[q + 1]]
        a = int(noff[2 * q]); seq[a:a + len(s)] = s; seq[a + len(s):a + 2 * len(s)] = _COMP[s[::-1]]
    return ReadSet(seq, None, noff)


def verify(api, queries, refs, cand_ref, cand_strand):
    """the candidates of Api.classify_search aligned: every query, oriented by its candidate's strand, against that reference, ONE Api.sg_align_cigar_batch call over
    all (query, candidate) pairs with match 2, mismatch -2, open 3, ext 1 -> dict of [n, top_k] arrays identity (float64), aln_cols, n_match (int32), q_cov, r_cov
    (float64); entries without a candidate are 0."""
    qs, rs = _as_readset(queries), _as_readset(refs)
    cand_ref = np.asarray(cand_ref); cand_strand = np.asarray(cand_strand)
    shape = cand_ref.shape
    out = dict(identity=np.zeros(shape), aln_cols=np.zeros(shape, np.int32), n_match=np.zeros(shape, np.int32), q_cov=np.zeros(shape), r_cov=np.zeros(shape))
    qi, ji = np.nonzero(cand_ref >= 0)
    if len(qi) == 0:
        return out
    used, t_idx = np.unique(cand_ref[qi, ji], return_inverse=True)                 # only the references that are somebody's candidate travel to the aligner
    sub = subset_reads(rs, used.astype(np.int64))
    q_idx = 2 * qi + cand_strand[qi, ji].astype(np.int64)
    _, cols = api.sg_align_cigar_batch(both_strands(qs), sub, q_idx, t_idx, ALN_OPEN, ext=ALN_EXT, match=ALN_MATCH, mismatch=ALN_MISMATCH)
    for q, j, c in zip(qi.tolist(), ji.tolist(), cols):
        d = identity_from_columns(c)
        for key in out:
            out[key][q, j] = d[key]
    return out


def rank(cand_ref, cand_shared, cand_strand, ver, min_identity=DEFAULTS["min_identity"], min_query_cov=DEFAULTS["min_query_cov"]):
    """per query the hits ordered by (identity descending, shared descending, ref ascending) -> one list per query of dicts(ref, strand, shared, identity, aln_cols,
    n_match, q_cov, r_cov, called); called = identity >= min_identity and q_cov >= min_query_cov"""
    cand_ref = np.asarray(cand_ref); out = []
    for q in range(cand_ref.shape[0]):
        js = [j for j in range(cand_ref.shape[1]) if cand_ref[q, j] >= 0]
        js.sort(key=lambda j: (-float(ver["identity"][q, j]), -int(cand_shared[q, j]), int(cand_ref[q, j])))
        out.append([dict(ref=int(cand_ref[q, j]), strand=int(cand_strand[q, j]), shared=int(cand_shared[q, j]), identity=float(ver["identity"][q, j]),
                         aln_cols=int(ver["aln_cols"][q, j]), n_match=int(ver["n_match"][q, j]), q_cov=float(ver["q_cov"][q, j]), r_cov=float(ver["r_cov"][q, j]),
                         called=bool(ver["identity"][q, j] >= min_identity and ver["q_cov"][q, j] >= min_query_cov)) for j in js])
    return out


def identify(api, refdb, queries, top_k=DEFAULTS["top_k"], min_shared=DEFAULTS["min_shared"], min_identity=DEFAULTS["min_identity"], min_query_cov=DEFAULTS["min_query_cov"]):
    """search + verify + rank of the sequences `queries` (strings or a host ReadSet, upper-case ACGTN) against the library behind refdb (Api.refdb_build keeps the
    reference sequences on the handle) -> the lists of rank()"""
    qs = _as_readset(queries)
    if qs.n == 0:
        return []
    ref, sh, st = api.classify_search(refdb, qs, top_k=top_k, min_shared=min_shared)
    return rank(ref, sh, st, verify(api, qs, refdb.refs, ref, st), min_identity, min_query_cov)


def n_reads_of(name):
    """the read count a consensus name of this tool carries (consensus_cl_id_X_total_supporting_reads_N), 0 for any other name"""
    m = re.search(r"_total_supporting_reads_(\d+)$", name)
    return int(m.group(1)) if m else 0


def table_rows(ids, n_reads, hits, library: Library, report=DEFAULTS["report"], sample=None):
    """the rows of classification.tsv: per consensus its first `report` hits (rank 1 ..), or one row with reference '*' when it has no candidate"""
    rows = []
    for cid, nr, hs in zip(ids, n_reads, hits):
        base = dict(consensus_id=cid, n_reads=int(nr))
        if sample is not None: base["sample"] = sample
        if not hs:
            rows.append(dict(base, rank=0, reference="*", strand="*", shared=0, identity=0.0, aln_cols=0, n_match=0, q_cov=0.0, r_cov=0.0, called=0, header="*"))
        for x, h in enumerate(hs[:max(int(report), 1)], 1):
            rows.append(dict(base, rank=x, reference=library.names[h["ref"]], strand="+-"[h["strand"]], shared=h["shared"], identity=h["identity"], aln_cols=h["aln_cols"],
                             n_match=h["n_match"], q_cov=h["q_cov"], r_cov=h["r_cov"], called=int(h["called"]), header=library.headers[h["ref"]]))
    return rows


def write_table(path, rows, with_sample=False):
    """tab-separated, one header line starting with '#'; floats as CPython's repr through the library's writer (fastio.repr_doubles), like the other tables"""
    cols = (("sample",) if with_sample else ()) + COLUMNS
    vals = np.array([r[c] for r in rows for c in _FLOATS], dtype=np.float64)
    buf, off = fastio.repr_doubles(vals)
    txt = [buf[int(off[i]):int(off[i + 1])].tobytes().decode() for i in range(len(vals))]
    with open(path, "w") as fh:
        fh.write("#" + "\t".join(cols) + "\n")
        for x, r in enumerate(rows):
            f = dict(zip(_FLOATS, txt[3 * x:3 * x + 3]))
            fh.write("\t".join(f[c] if c in f else str(r[c]) for c in cols) + "\n")


def check_args(args):
    """the range checks of the --classify_* flags -> an error text or None"""
    if not 1 <= args.classify_k <= CLASSIFY_MAX_K:
        return "--classify_k must be 1..%d (minimizer codes of larger k are not comparable between a library and a query)." % CLASSIFY_MAX_K
    if not args.classify_k <= args.classify_w <= 255:
        return "--classify_w must be at least --classify_k and at most 255."
    if not 1 <= args.classify_top_k <= CLASSIFY_MAX_TOPK:
        return "--classify_top_k must be 1..%d." % CLASSIFY_MAX_TOPK
    if args.classify_min_shared < 1:
        return "--classify_min_shared must be at least 1."
    if not (0.0 <= args.classify_min_identity <= 1.0 and 0.0 <= args.classify_min_query_cov <= 1.0):
        return "--classify_min_identity and --classify_min_query_cov are fractions in [0, 1]."
    if args.classify_report < 1:
        return "--classify_report must be at least 1."
    return None


def add_flags(p):
    """the --classify_* flags, shared by the main command and the `classify` sub-command"""
    d = DEFAULTS
    p.add_argument('--classify_k', type=int, default=d["k"], help='extension: minimizer k of the library search (1..21)')
    p.add_argument('--classify_w', type=int, default=d["w"], help='extension: minimizer window of the library search')
    p.add_argument('--classify_top_k', type=int, default=d["top_k"], help='extension: candidate references per consensus that are verified by alignment (1..64)')
    p.add_argument('--classify_min_shared', type=int, default=d["min_shared"], help='extension: a reference sharing fewer minimizers with a consensus is no candidate')
    p.add_argument('--classify_min_identity', type=float, default=d["min_identity"], help='extension: a hit is called at this alignment identity or above (a policy default, not a measurement)')
    p.add_argument('--classify_min_query_cov', type=float, default=d["min_query_cov"], help='extension: ... and when at least this share of the consensus lies inside the alignment (a policy default)')
    p.add_argument('--classify_report', type=int, default=d["report"], help='extension: rows written per consensus')


def run(args, api, groups, library=None):
    """the --reference_db step: groups = [(sample name or None, folder, [(consensus id, n_reads, sequence)])].  The consensuses of ALL groups are searched in one
    Api.classify_search call and verified in one aligner call; every folder gets classification.tsv, and with sample names <outfolder>/classification_all.tsv holds
    all rows behind a leading sample column.  -> rows per group"""
    library = library or read_reference_fasta(args.reference_db)
    seqs = [s for _, _, cons in groups for _, _, s in cons]
    with api.refdb_build(library.rs, k=args.classify_k, w=args.classify_w) as db:
        hits = identify(api, db, seqs, top_k=args.classify_top_k, min_shared=args.classify_min_shared, min_identity=args.classify_min_identity, min_query_cov=args.classify_min_query_cov)
    import os
    out, x, everything = [], 0, []
    for sample, folder, cons in groups:
        rows = table_rows([c[0] for c in cons], [c[1] for c in cons], hits[x:x + len(cons)], library, report=args.classify_report, sample=sample)
        x += len(cons)
        write_table(os.path.join(folder, "classification.tsv"), rows)
        out.append(rows); everything.extend(rows)
    if any(sample is not None for sample, _, _ in groups):
        write_table(os.path.join(args.outfolder, "classification_all.tsv"), everything, with_sample=True)
    return out


def classify_fasta(args, api=None):
    """the `classify` sub-command: any FASTA against a library -> args.outfile (the table of --reference_db; n_reads from names of this tool's consensuses, else 0)"""
    from . import runtime
    api = api or runtime.get_api()
    q = read_reference_fasta(args.fasta, unique_names=False)
    library = read_reference_fasta(args.reference_db)
    with api.refdb_build(library.rs, k=args.classify_k, w=args.classify_w) as db:
        hits = identify(api, db, q.rs, top_k=args.classify_top_k, min_shared=args.classify_min_shared, min_identity=args.classify_min_identity, min_query_cov=args.classify_min_query_cov)
    rows = table_rows(q.names, [n_reads_of(n) for n in q.names], hits, library, report=args.classify_report)
    write_table(args.outfile, rows)
    return rows
