"""Homopolymer finishing pass (extension, off by default): a run-length vote over the reads, NOT medaka.

Api.hp_runs (include/ngsid_hp.h) counts, per homopolymer run of a consensus and per strand, how long that run is in every read that spans it between two matching flanks.
This module is the policy on top of those integers: which runs to list (runs), which length a histogram calls (call), the rewritten sequence (apply) and the rounds
(polish).  Letters never change and no run is removed, so neighbouring runs never merge and the run list of a sequence keeps its order.

The calling rule has one fixed shape; its thresholds were swept on the CPU reference (tools/hp_sweep.py, profiles/hp.txt):
  - a length is called only between 1 and MAX_CALL (the exact buckets of the histogram);
  - the usable depth (reads in the length buckets, both strands) is at least min_depth;
  - the called length is the mode of the two strands together, alone at the top;
  - it holds at least min_share of the usable depth and leads the centre's own length by at least min_margin of it;
  - it is never called against a strand that has min_strand_depth usable reads of its own and does not prefer the called length to the centre's."""
import numpy as np
from ._capi import ReadSet, HP_NBUCKET, HP_OTHER

MAX_CALL = 14                   # buckets 0 .. 14 are exact lengths, 15 is "15 or more"
DEFAULTS = dict(min_depth=8, min_share=0.6, min_margin=0.2, min_strand_depth=4)      # profiles/hp.txt: the row of the grid that meets both conditions with the veto on and the margin of the prototype


def runs(seq):
    """-> (starts uint32, lengths int64): every maximal run of equal bytes of seq, in order (runs of one base included: a run the centre has as one base can be two)"""
    b = np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), dtype=np.uint8)
    if len(b) == 0:
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int64)
    starts = np.concatenate(([0], np.nonzero(b[1:] != b[:-1])[0] + 1))
    return starts.astype(np.uint32), np.diff(np.concatenate((starts, [len(b)]))).astype(np.int64)


def call(hist, run_len, min_depth=DEFAULTS["min_depth"], min_share=DEFAULTS["min_share"], min_margin=DEFAULTS["min_margin"], min_strand_depth=DEFAULTS["min_strand_depth"]):
    """hist [n, 2, HP_NBUCKET] of Api.hp_runs, run_len [n] the lengths the centre has -> new length per run (== run_len where nothing is called)"""
    hist = np.asarray(hist, dtype=np.int64).reshape(-1, 2, HP_NBUCKET); run_len = np.asarray(run_len, dtype=np.int64)
    out = run_len.copy()
    for i in range(len(run_len)):
        both = hist[i, 0, :HP_OTHER] + hist[i, 1, :HP_OTHER]
        depth = int(both.sum())
        if depth < min_depth or depth == 0: continue
        L = int(both.argmax()); own = min(int(run_len[i]), HP_OTHER - 1)
        if L == own or L < 1 or L > MAX_CALL: continue
        if (both == both[L]).sum() > 1: continue                                   # a tie at the top is no mode
        if both[L] < min_share * depth or both[L] - both[own] < min_margin * depth: continue
        veto = False
        for s in (0, 1):
            hs = hist[i, s, :HP_OTHER]
            if hs.sum() >= max(min_strand_depth, 1) and hs[own] >= hs[L]: veto = True
        if not veto: out[i] = L
    return out


def apply(seq, starts, new_len):
    """seq with the runs that begin at starts (ascending first positions of maximal runs) set to new_len bases each; every other base stays"""
    st, ln = runs(seq)
    want = dict(zip((int(x) for x in starts), (int(x) for x in new_len)))
    missing = set(want) - set(int(x) for x in st)
    if missing: raise ValueError("hp.apply: %s are not first positions of runs" % sorted(missing))
    if any(v < 1 for v in want.values()): raise ValueError("hp.apply: a run cannot be removed")
    return "".join(seq[int(a)] * want.get(int(a), int(n)) for a, n in zip(st, ln))


def polish(api, seqs, rs, lists, k=13, w=20, rounds=2, clip=False, **thresholds):
    """The pass over the sequences seqs with their read lists (read numbers of rs): per round ONE Api.hp_runs call for all sequences that changed in the round before (all of
    them in the first), call() on every run, apply().  Stops when nothing changes.
    -> (new sequences, changes): changes[i] = list of dict(round, pos (in the sequence that round saw), letter, old, new, hist [2, HP_NBUCKET]) of sequence i."""
    seqs = list(seqs); changes = [[] for _ in seqs]
    live = [i for i, q in enumerate(seqs) if len(q) and len(lists[i])]
    for rnd in range(rounds):
        if not live: break
        rl = [runs(seqs[i]) for i in live]
        run_off = np.concatenate(([0], np.cumsum([len(s) for s, _ in rl]))).astype(np.uint64)
        ll = [np.asarray(lists[i], dtype=np.uint32) for i in live]
        grp_off = np.concatenate(([0], np.cumsum([len(x) for x in ll]))).astype(np.uint64)
        hist, _ = api.hp_runs(ReadSet.from_strings([seqs[i] for i in live]), rs, grp_off, run_off, np.concatenate([s for s, _ in rl]), read_order=np.concatenate(ll), k=k, w=w, clip=clip)
        nxt = []
        for j, i in enumerate(live):
            st, ln = rl[j]; h = hist[int(run_off[j]):int(run_off[j + 1])]
            new = call(h, ln, **thresholds)
            ch = np.nonzero(new != ln)[0]
            if len(ch) == 0: continue
            for x in ch:
                changes[i].append(dict(round=rnd, pos=int(st[x]), letter=seqs[i][int(st[x])], old=int(ln[x]), new=int(new[x]), hist=h[x].copy()))
            seqs[i] = apply(seqs[i], st[ch], new[ch]); nxt.append(i)
        live = nxt
    return seqs, changes


def policy_from_args(args):
    """the keyword arguments of polish() from the command line's --hp_* flags"""
    return dict(rounds=args.hp_rounds, min_depth=args.hp_min_depth, min_share=args.hp_min_share, min_margin=args.hp_min_margin, min_strand_depth=args.hp_min_strand_depth)


TABLE_HEADER = ("cluster_id", "pos", "letter", "old_len", "new_len", "round", "hist_plus", "hist_minus")


def table_rows(ids, changes):
    """rows of hp_polish.tsv: one per changed run, in centre order; the two strand histograms as 17 comma-separated counts (lengths 0 - 14, 15 or more, no length)"""
    return [(str(c_id), str(c["pos"]), c["letter"], str(c["old"]), str(c["new"]), str(c["round"]), ",".join(str(int(v)) for v in c["hist"][0]), ",".join(str(int(v)) for v in c["hist"][1]))
            for c_id, ch in zip(ids, changes) for c in ch]


def write_table(path, rows, header=TABLE_HEADER):
    with open(path, "w") as f:
        f.write("\t".join(header) + "\n")
        for r in rows: f.write("\t".join(r) + "\n")
