"""Flagging PCR chimeras among the consensuses of a sample (extension; `--chimeras`, sub-command `chimeras`): the policy on top of ngsid_chimera_model
(include/ngsid_chimera.h, csrc/k_chimera.hip).

The library returns, per consensus, the edit distance of its best one-parent model and of its best two-parent model (head from one parent, tail from another) over the
parents it is offered, as integers.  Which consensuses are offered as parents (the more abundant ones of the same sample, both strands, UCHIME's abundance skew), and
which result is called a chimera (the gain of the second parent, the distance that is left, a breakpoint inside the sequence), is decided here, and the table is written here.

The default thresholds come from tools/chimera_sweep.py over tests/chimera_reference.py (profiles/chimera.txt): no sequence of the non-chimeric
sets is called at them.  min_abskew = 2.0 is UCHIME's published default.
"""
from __future__ import annotations
import os
import numpy as np
from . import classify
from ._capi import ReadSet, CHIMERA_FIELDS

DEFAULTS = dict(min_abskew=2.0, min_gain=5, max_model_frac=0.005)
COLUMNS = ("id", "n_reads", "length", "chimeric", "best_parent", "best_strand", "best_ed", "parent_a", "strand_a", "parent_b", "strand_b", "model_ed", "gain", "bp_lo", "bp_hi")
_F = {name: x for x, name in enumerate(CHIMERA_FIELDS)}


def candidates(sizes, min_abskew=DEFAULTS["min_abskew"]):
    """the pairs of ONE sample: parent p is offered to query q (p != q) when sizes[p] >= min_abskew * sizes[q], on both strands -> (pair_off [n + 1] uint64,
    pair_parent uint32, pair_gid int32).  pair_parent indexes classify.both_strands of the sample's sequences (2 p = p forward, 2 p + 1 = its reverse complement);
    the two strands of a parent share the gid p, so no model glues a parent to its own reverse complement.  Parents in ascending index order, forward strand first."""
    sizes = np.asarray(sizes, dtype=np.float64)
    n = len(sizes)
    pair_off = np.zeros(n + 1, dtype=np.uint64); parent, gid = [], []
    for q in range(n):
        ps = [p for p in range(n) if p != q and sizes[p] >= min_abskew * sizes[q]]
        for p in ps:
            parent += [2 * p, 2 * p + 1]; gid += [p, p]
        pair_off[q + 1] = len(parent)
    return pair_off, np.asarray(parent, dtype=np.uint32), np.asarray(gid, dtype=np.int32)


def call(fields, lengths, min_gain=DEFAULTS["min_gain"], max_model_frac=DEFAULTS["max_model_frac"]):
    """fields [n, 7] of Api.chimera_model, lengths [n] -> bool [n]: q is chimeric when a two-parent model exists (two_cost >= 0), the second parent gains at least
    min_gain edits (one_cost - two_cost >= min_gain), the model is close (two_cost <= max_model_frac * length) and its breakpoint interval lies inside the sequence
    (0 < bp_lo and bp_hi < length: a model that takes everything from one parent is no chimera)"""
    f = np.asarray(fields).reshape(-1, len(CHIMERA_FIELDS)).astype(np.int64); n = np.asarray(lengths, dtype=np.int64)
    two, one = f[:, _F["two_cost"]], f[:, _F["one_cost"]]
    return (two >= 0) & (one - two >= min_gain) & (two.astype(np.float64) <= max_model_frac * n.astype(np.float64)) & (f[:, _F["bp_lo"]] > 0) & (f[:, _F["bp_hi"]] < n)


def model(api, seqs, sizes, sample_off=None, min_abskew=DEFAULTS["min_abskew"]):
    """ONE Api.chimera_model call over the sequences of all samples: seqs [n] strings, sizes [n] read counts, sample s = [sample_off[s], sample_off[s + 1]) (None: one
    sample).  Parents are offered within a sample only.  -> (fields [n, 7], pair_off [n + 1], pair_parent, pair_gid) with pair_parent = 2 * sequence + strand and gid =
    sequence, both numbered over ALL sequences"""
    n = len(seqs)
    so = [0, n] if sample_off is None else [int(x) for x in sample_off]
    offs, parents, gids = [np.zeros(1, dtype=np.uint64)], [], []
    for a, b in zip(so[:-1], so[1:]):
        po, pp, pg = candidates(sizes[a:b], min_abskew)
        offs.append(po[1:] + offs[-1][-1]); parents.append(pp + np.uint32(2 * a)); gids.append(pg + np.int32(a))
    pair_off = np.concatenate(offs)
    pair_parent = np.concatenate(parents) if parents else np.zeros(0, np.uint32); pair_gid = np.concatenate(gids) if gids else np.zeros(0, np.int32)
    qs = ReadSet.from_strings(list(seqs))
    fields = api.chimera_model(qs, classify.both_strands(qs), pair_off, pair_parent, pair_gid) if n else np.zeros((0, len(CHIMERA_FIELDS)), np.int32)
    return fields, pair_off, pair_parent, pair_gid


def describe(fields, pair_off, pair_parent, lengths, called, base=0):
    """one dict per query: chimeric, length, best_parent / best_strand / best_ed (one-parent model), parent_a / strand_a / parent_b / strand_b / model_ed / gain / bp_lo /
    bp_hi (two-parent model); parents as sequence numbers minus `base` (the sample's first sequence), strands 0 / 1, -1 where a model does not exist"""
    out = []
    for q in range(len(fields)):
        f = [int(x) for x in fields[q]]; a0 = int(pair_off[q])
        def who(k):
            if k < 0: return -1, -1
            p = int(pair_parent[a0 + k]); return p // 2 - base, p % 2
        bp, bs = who(f[_F["one_pair"]]); pa, sa = who(f[_F["pair_a"]]); pb, sb = who(f[_F["pair_b"]])
        two = f[_F["two_cost"]]
        out.append(dict(chimeric=bool(called[q]), length=int(lengths[q]), best_parent=bp, best_strand=bs, best_ed=f[_F["one_cost"]], parent_a=pa, strand_a=sa, parent_b=pb, strand_b=sb,
                        model_ed=two, gain=(f[_F["one_cost"]] - two) if two >= 0 else -1, bp_lo=f[_F["bp_lo"]], bp_hi=f[_F["bp_hi"]]))
    return out


def detect(api, seqs, sizes, sample_off=None, min_abskew=DEFAULTS["min_abskew"], min_gain=DEFAULTS["min_gain"], max_model_frac=DEFAULTS["max_model_frac"]):
    """model + call + describe -> one list of dicts per sample (parents numbered within the sample)"""
    n = len(seqs)
    so = [0, n] if sample_off is None else [int(x) for x in sample_off]
    fields, pair_off, pair_parent, _ = model(api, seqs, np.asarray(sizes), so, min_abskew)
    lengths = np.array([len(s) for s in seqs], dtype=np.int64)
    called = call(fields, lengths, min_gain, max_model_frac)
    return [describe(fields[a:b], pair_off[a:b + 1], pair_parent, lengths[a:b], called[a:b], base=a) for a, b in zip(so[:-1], so[1:])]


def table_rows(ids, n_reads, entries, sample=None):
    """the rows of chimeras.tsv: one per consensus; parents by their ids, strands as + / -, '*' and -1 where a model does not exist"""
    rows = []
    name = lambda p: ids[p] if p >= 0 else "*"
    strand = lambda s: "+-"[s] if s >= 0 else "*"
    for cid, nr, e in zip(ids, n_reads, entries):
        r = dict(id=cid, n_reads=int(nr), length=e["length"], chimeric=int(e["chimeric"]), best_parent=name(e["best_parent"]), best_strand=strand(e["best_strand"]), best_ed=e["best_ed"],
                 parent_a=name(e["parent_a"]), strand_a=strand(e["strand_a"]), parent_b=name(e["parent_b"]), strand_b=strand(e["strand_b"]), model_ed=e["model_ed"], gain=e["gain"],
                 bp_lo=e["bp_lo"], bp_hi=e["bp_hi"])
        if sample is not None: r["sample"] = sample
        rows.append(r)
    return rows


_INTS = ("n_reads", "length", "chimeric", "best_ed", "model_ed", "gain", "bp_lo", "bp_hi")


def write_table(path, rows, with_sample=False):
    """tab-separated, one header line starting with '#', like the other tables"""
    cols = (("sample",) if with_sample else ()) + COLUMNS
    with open(path, "w") as fh:
        fh.write("#" + "\t".join(cols) + "\n")
        for r in rows:
            fh.write("\t".join(str(r[c]) for c in cols) + "\n")


def read_table(path):
    """the rows write_table wrote (integers as integers; a sample column when the table has one)"""
    with open(path) as fh:
        cols = fh.readline().rstrip("\n").lstrip("#").split("\t")
        return [{c: (int(v) if c in _INTS else v) for c, v in zip(cols, line.rstrip("\n").split("\t"))} for line in fh if line.strip()]


def check_args(args):
    """the range checks of the --chimera_* flags -> an error text or None"""
    if not args.chimera_min_abskew > 0.0:
        return "--chimera_min_abskew must be positive (a parent has at least this many times the reads of the consensus it explains)."
    if args.chimera_min_gain < 1:
        return "--chimera_min_gain must be at least 1 (a second parent that saves no edit explains nothing)."
    if not 0.0 <= args.chimera_max_model_frac <= 1.0:
        return "--chimera_max_model_frac is a fraction in [0, 1]."
    return None


def add_flags(p):
    """the --chimera_* flags, shared by the main command and the `chimeras` sub-command"""
    d = DEFAULTS
    p.add_argument('--chimera_min_abskew', type=float, default=d["min_abskew"], help='extension: a consensus is offered as a parent to one with at most 1 / this of its reads (UCHIME\'s abundance skew)')
    p.add_argument('--chimera_min_gain', type=int, default=d["min_gain"], help='extension: a consensus is chimeric when its best two-parent model is at least this many edits closer than its best single parent')
    p.add_argument('--chimera_max_model_frac', type=float, default=d["max_model_frac"], help='extension: ... and when that model is within this fraction of the consensus length in edits')


def _kwargs(args):
    return dict(min_abskew=args.chimera_min_abskew, min_gain=args.chimera_min_gain, max_model_frac=args.chimera_max_model_frac)


def run(args, api, groups):
    """the --chimeras step: groups = [(sample name or None, folder, [(consensus id, n_reads, sequence)])].  The consensuses of ALL groups are modelled in one
    Api.chimera_model call (parents within a group only); every folder gets chimeras.tsv, and with sample names <outfolder>/chimeras_all.tsv holds all rows behind a
    leading sample column.  -> rows per group"""
    seqs = [s for _, _, cons in groups for _, _, s in cons]
    sizes = [nr for _, _, cons in groups for _, nr, _ in cons]
    so = np.concatenate(([0], np.cumsum([len(cons) for _, _, cons in groups]))).astype(np.int64)
    per = detect(api, seqs, sizes, so, **_kwargs(args))
    out, everything = [], []
    for (sample, folder, cons), entries in zip(groups, per):
        rows = table_rows([c[0] for c in cons], [c[1] for c in cons], entries, sample=sample)
        write_table(os.path.join(folder, "chimeras.tsv"), rows)
        out.append(rows); everything.extend(rows)
    if any(sample is not None for sample, _, _ in groups):
        write_table(os.path.join(args.outfolder, "chimeras_all.tsv"), everything, with_sample=True)
    return out


def chimeras_fasta(args, api=None):
    """the `chimeras` sub-command: the sequences of any FASTA as one sample -> args.outfile (the table of --chimeras; read counts from names of this tool's consensuses, else 0)"""
    from . import runtime
    api = api or runtime.get_api()
    q = classify.read_reference_fasta(args.fasta, unique_names=False)
    seqs = [q.rs.get(i)[0] for i in range(q.rs.n)]
    sizes = [classify.n_reads_of(n) for n in q.names]
    rows = table_rows(q.names, sizes, detect(api, seqs, sizes, None, **_kwargs(args))[0])
    write_table(args.outfile, rows)
    return rows
