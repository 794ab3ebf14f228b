"""A plain reference of ngsid_polish / ngsid_polish_trace / ngsid_polish_trace_aln for aln_mode 1 / 2 and 3, ONE group at a time, every window ONE graph in racon's
order (backbone, then the layers by first position), numpy and the standard library only.  Written from include/ngsid.h ("THE RULES OF ONE POLISHING ITERATION") and
racon's published rules; it shares no code with oracle/ or the library and stands on the two anchors that already exist: ed_reference.py (read -> backbone alignment)
and poa_reference.py (one graph, heaviest bundle, `decided`).  What it pins is the glue between them: strand call, orientation, PAF records, window geometry, layer
filters, layer mode, layer order, the zero-weight backbone, trimming, stitching, n_used and the iteration over a backbone whose length changes.

subgraph=True is the flag bit NGSID_ALN_SUBGRAPH of aln_mode (racon's sub-graph layers, as the header defines them).
Not modelled: aln_mode 0, windows built as tile hierarchies, band redo, capacity splits - and stop_when_stable, which changes no output (the
polisher is a function of (backbone, reads); tests assert that the two settings agree).

Trim: for ONE graph per window the window rule below is the whole rule.  With trim == 2 the library also trims the consensus of the (single) tile, with the same
threshold (half the layers merged) on the same coverage: the window trim that follows finds the ends already there, the second application is idempotent.

polish_reference(...) -> (seqs[it], used[it], aln[it] (int32 [n_reads, 6]), decided, info); decided = AND of poa_reference's `decided` over all windows and iterations;
info = {"reads": [(a, b, strand)], "tgs": bool, "nwin": [per iteration], "layers": [(iteration, read, window, qf, ql, begin, end, mode, status)] with status "kept" /
"short" / "quality", "span_dropped": [(iteration, read, mn, mx)], "unclipped": [(iteration, read)] (aln_mode 3: no run of 15 equal columns),
"windows": [(iteration, window, layers, trimmed bases in front, behind)]}.
"""
import numpy as np
import ed_reference as ed
import poa_reference as poa

GLOBAL, SEMI = poa.GLOBAL, poa.SEMI
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
DEFAULTS = dict(iters=2, window=500, quality_threshold=10.0, error_threshold=0.3, match=3, mismatch=-5, gap=-4, k=13, w=20, trim=1, aln_mode=2, subgraph=False)


def revcomp(s):
    return "".join(_COMP.get(c, "N") for c in reversed(s))


# ---- 1. strand
def hpc(s):
    return "".join(c for i, c in enumerate(s) if i == 0 or c != s[i - 1])


def minimizers(s, k, w):
    """the emitted minimizer k-mers of the homopolymer-compressed string, as strings, in order (repeats included).  Python compares strings byte-wise: A < C < G < N < T,
    and a slice that runs past the end is a proper prefix and so sorts first."""
    h = hpc(s)
    if len(h) < k: return []
    per = w - k + 1
    nk = len(h) - k + 1
    kmers = [h[i:i + k] for i in range(max(nk, per))]
    out, prev = [], -1
    for start in range(max(nk - per + 1, 1)):
        win = kmers[start:start + per]
        best = start + win.index(min(win))             # index() finds the first = leftmost minimum
        if best != prev:
            out.append(kmers[best]); prev = best
    return out


def strand_call(read, fwd, rev, k, w):
    """-> (a, b, strand): strand 0 plus, 1 minus, -1 not used"""
    mz = minimizers(read, k, w)
    a = sum(1 for x in mz if x in fwd); b = sum(1 for x in mz if x in rev)
    return a, b, (-1 if a == 0 and b == 0 else (1 if b > a else 0))


# ---- 2. alignment
def clip_to_runs(cols, q, t, run=15):
    """aln_mode 3: the diagonal columns from the first to the last run of >= `run` consecutive equal columns (a gap column ends a run)"""
    first = last = None; n = 0
    for x in range(len(cols)):
        qi, ti = int(cols[x, 0]), int(cols[x, 1])
        eq = q[qi] in "ACGTacgt" and q[qi].upper() == t[ti].upper()
        adjacent = x > 0 and int(cols[x - 1, 0]) == qi - 1 and int(cols[x - 1, 1]) == ti - 1
        n = (n + 1 if adjacent else 1) if eq else 0
        if n >= run:
            if first is None: first = x - run + 1
            last = x
    return cols[:0] if first is None else cols[first:last + 1]


# ---- 3. windows
def nwin(Bl, W):
    raw = 1 if Bl <= W else -(-Bl // W)
    tail = Bl - (raw - 1) * W
    return raw - 1 if raw >= 2 and tail < W // 10 else raw


def wlen(Bl, W, w):
    return Bl - w * W if w == nwin(Bl, W) - 1 else W


# ---- 5. one window
def window_consensus(slice_, layers, match, mismatch, gap, subgraph=False):
    """layers: [(sequence, weights, mode, begin, end)] in graph order -> (consensus, coverage, decided).  subgraph (NGSID_ALN_SUBGRAPH): a layer that does not span
    its window is aligned GLOBALLY to the sub-graph of its backbone positions [begin, end] instead of end-free to the whole graph"""
    G = poa.Graph(); decided = True
    s = slice_.encode()
    G.add_sequence(s, [0] * len(s), {}, counted=False)
    for sq, wts, mode, begin, end in layers:
        s = sq.encode()
        if subgraph and mode == SEMI: outcome, ok = poa.align(G, s, GLOBAL, match, mismatch, gap, enumerate_all=decided, within=poa.subgraph_nodes(G, begin, end))
        else: outcome, ok = poa.align(G, s, mode, match, mismatch, gap, enumerate_all=decided)
        decided = decided and ok
        G.add_sequence(s, wts, outcome)
    path, ok = poa.heaviest_bundle(G, chain_ties=True)
    cons = bytes(G.letter[v] for v in path).decode()
    cov = [sum(G.count[u] for u in G.sib[v]) for v in path]
    return cons, cov, decided and ok


def polish_reference(backbone, reads, quals=None, **kw):
    P = dict(DEFAULTS); P.update(kw)
    assert P["aln_mode"] in (1, 2, 3)
    W = P["window"]; n_reads = len(reads)
    info = {"reads": [], "layers": [], "span_dropped": [], "unclipped": [], "windows": [], "nwin": []}
    # 1. strand, once, against the initial backbone
    k1 = min(P["k"], 21); w1 = max(P["w"], k1)
    fwd = set(minimizers(backbone, k1, w1)); rev = set(minimizers(revcomp(backbone), k1, w1))
    oriented = []
    for x, r in enumerate(reads):
        a, b, st = strand_call(r, fwd, rev, k1, w1)
        info["reads"].append((a, b, st))
        if st < 0: oriented.append(None)
        elif st == 0: oriented.append((r, None if quals is None else quals[x]))
        else: oriented.append((revcomp(r), None if quals is None else quals[x][::-1]))
    tgs = n_reads > 0 and sum(len(r) for r in reads) / n_reads > 1000.0
    info["tgs"] = tgs
    trimming = P["trim"] == 2 or (P["trim"] in (1, 3) and tgs)
    B = backbone; decided = True
    seqs, used, aln = [], [], []
    for it in range(P["iters"]):
        Bl = len(B); nw = nwin(Bl, W); info["nwin"].append(nw)
        rec = np.full((n_reads, 6), -1, dtype=np.int32)
        per_window = [[] for _ in range(nw)]
        n_used = 0
        for x in range(n_reads):
            if oriented[x] is None: continue
            r, q = oriented[x]; n = len(r)
            # 2. alignment against the CURRENT backbone
            dist, _, cols = ed.align_pair(r, B)
            if P["aln_mode"] == 3:
                cols = clip_to_runs(cols, r, B)
                if not len(cols): info["unclipped"].append((it, x))
            if not len(cols): continue
            qb, qe, tb, te = int(cols[0, 0]), int(cols[-1, 0]), int(cols[0, 1]), int(cols[-1, 1])
            minus = info["reads"][x][2] == 1
            rec[x] = (int(minus), n - 1 - qe if minus else qb, n - qb if minus else qe + 1, tb, te + 1, dist)
            # 4. the read as a whole
            qs, ts = qe - qb + 1, te - tb + 1
            mn, mx = min(qs, ts), max(qs, ts)
            if 1.0 - mn / mx > P["error_threshold"]:
                info["span_dropped"].append((it, x, mn, mx)); continue
            # 3. + 4. its layers
            win_of = np.minimum(cols[:, 1] // W, nw - 1)
            contributed = False
            for w in range(nw):
                sel = np.nonzero(win_of == w)[0]
                if not len(sel): continue
                qf, ql, tf, tl = int(cols[sel[0], 0]), int(cols[sel[-1], 0]), int(cols[sel[0], 1]), int(cols[sel[-1], 1])
                ln = ql - qf + 1
                wl = wlen(Bl, W, w)
                begin, end = tf - w * W, tl - w * W
                offset = int(0.01 * wl)
                mode = GLOBAL if begin < offset and end > wl - offset else SEMI
                status = "kept"
                if ln < 0.02 * W: status = "short"
                elif q is not None and sum(ord(c) - 33 for c in q[qf:ql + 1]) / ln < P["quality_threshold"]: status = "quality"
                info["layers"].append((it, x, w, qf, ql, begin, end, mode, status))
                if status != "kept": continue
                wts = [1] * ln if q is None else [ord(c) - 33 for c in q[qf:ql + 1]]
                per_window[w].append((begin, r[qf:ql + 1], wts, mode, begin, end)); contributed = True
            n_used += contributed
        # 5. - 7. the windows, stitched
        parts = []
        for w in range(nw):
            wl = wlen(Bl, W, w); piece = B[w * W:w * W + wl]
            L = sorted(per_window[w], key=lambda e: e[0])                  # sorted() is stable: equal `begin` keeps the listed read order
            if len(L) >= 2:
                cons, cov, ok = window_consensus(piece, [e[1:] for e in L], P["match"], P["mismatch"], P["gap"], P["subgraph"])
                decided = decided and ok
                front = behind = 0
                if trimming and cons:
                    thr = len(L) // 2
                    ok_pos = [i for i, c in enumerate(cov) if c >= thr]
                    if ok_pos and ok_pos[0] < ok_pos[-1]:
                        front, behind = ok_pos[0], len(cons) - 1 - ok_pos[-1]
                        cons = cons[ok_pos[0]:ok_pos[-1] + 1]
                info["windows"].append((it, w, len(L), front, behind))
                if cons: piece = cons
            else:
                info["windows"].append((it, w, len(L), 0, 0))
            parts.append(piece)
        B = "".join(parts)
        seqs.append(B); used.append(n_used); aln.append(rec)
    return seqs, used, aln, decided, info
