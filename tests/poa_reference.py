"""A plain reference of ngsid_poa_consensus / _cov / _weighted for ONE group as ONE graph in file order (tile_depth <= 0, trim = 0), numpy and the
standard library only, written from include/ngsid.h and the published spoa algorithm (Vaser et al. 2017; Lee et al. 2002 for the heaviest bundle)
and sharing no code with oracle/ or the library - the anchor that oracle and kernel are both compared with.

What it does differently from the oracle ON PURPOSE: no band (every node x every column), no incremental rank scheme (the topological order is
recomputed from scratch by Kahn's algorithm for every alignment and for the consensus), no in-edge slots or edge lists (in-edges are a dict), and no
traceback direction matrix: the traceback is found afterwards from the score matrix, and ALL co-optimal tracebacks are enumerated.

Graph.  A node has a letter, in-edges {predecessor: weight}, successors, the set of its aligned siblings (one shared set object per alignment column,
the node included) and the number of sequences that pass through it.  A sequence adds w[i-1] + w[i] to the edge between its bases i-1 and i;
w = qual - 33 (FASTQ), 1 (FASTA, qual None) or min(max(weight, 1), 2^20) for the weighted entry point (qualities ignored).

Alignment (linear gap g, match m, mismatch n; row = node, column j = j bases consumed):
  LOCAL   scores clamped at 0, an alignment starts at any node, ends at the maximum over all cells and is traced back until a cell of score 0 (Smith-
          Waterman: a traceback stops at the first 0, that is the algorithm and no tie); bases in front of and behind it become new branches; with
          no positive cell the whole sequence is a new branch.
  GLOBAL  a virtual source row S[j] = j g stands in front of the nodes without a predecessor; ends in the last column at a node without successor.
  SEMI    the diagonal from S[j-1] is open to EVERY node, there is no vertical move from the source; ends in the last column at any node.
Adding: an aligned node with the base's letter is reused; else the sibling with that letter; else a new node joins the sibling set.

Consensus: heaviest bundle.  In topological order every node takes its in-edge of maximum weight (equal weights: the predecessor with the larger
score), score = that weight + the predecessor's score, a node without in-edge scores -1; start at the node of maximum score; while that node has
successors apply spoa's branch completion (the OTHER predecessors of its successors are invalidated (-1), every node behind it in the order is
scored again without edges from invalidated nodes, the new maximum among those takes over); backtrack along the chosen predecessors.
cov[x] = sum over the sibling set of consensus node x of the number of sequences through each node.

`decided`.  POA results depend on tie-breaks that are build choices (rank order, edge-list order).  The reference reports when ITS result depended on
one - from the graph and the scores alone, before any other implementation's output is looked at:
  alignment   every co-optimal traceback from every co-optimal end cell is enumerated (depth first, states de-duplicated on (node, column, pairs so
              far); more than PATH_CAP branches = undecided).  A traceback is mapped to its OUTCOME: for every aligned base the node that adding would
              reuse, or ("new", smallest id of the sibling set).  More than one distinct outcome = undecided.  (Paths that skip either of two siblings,
              or mismatch against either, differ as paths and give the same graph: they are one outcome.)
  consensus   two best in-edges of a node with equal weight and equal predecessor score; the maximum score attained by more than one node; the same
              inside branch completion; and a branch completion whose result depends on the topological order: spoa scores "every node of higher rank"
              again there (and in that pass, unlike in the first, skips edges from nodes that score -1, sources included), so for a node that is neither
              an ancestor nor a descendant of the node being completed it is the order that says whether it is scored again.  The completion is run
              with none and with all of those nodes scored again; two different consensus paths = undecided.
After the first undecided event the rest of the group is computed along the first traceback found (the result is not used for comparisons).

Hooks for polish_reference.py (a polishing window is such a graph with the backbone in front), all off by default: add_sequence(counted=False) - a first sequence
that no coverage counts; align(within=nodes) with subgraph_nodes() - an alignment that sees a node set only (global to racon's sub-graph of a layer);
heaviest_bundle(chain_ties=True) - a maximum repeated along one simple chain is no tie.
"""
from collections import deque
import numpy as np

LOCAL, GLOBAL, SEMI = 0, 1, 2
NEG = -(1 << 40)
PATH_CAP = 4096
WEIGHT_CAP = 1 << 20


class Graph:
    def __init__(self):
        self.letter, self.inn, self.out, self.sib, self.count = [], [], [], [], []

    def new_node(self, c, sibling_of=None):
        y = len(self.letter)
        self.letter.append(c); self.inn.append({}); self.out.append([]); self.count.append(0)
        if sibling_of is None: self.sib.append({y})
        else:
            s = self.sib[sibling_of]; s.add(y); self.sib.append(s)
        return y

    def add_edge(self, a, b, w):
        if a in self.inn[b]: self.inn[b][a] += w
        else:
            self.inn[b][a] = w; self.out[a].append(b)

    def topo(self):
        """Kahn's algorithm from scratch; raises on a cycle"""
        n = len(self.letter)
        deg = [len(d) for d in self.inn]
        q = deque(v for v in range(n) if deg[v] == 0)
        order = []
        while q:
            v = q.popleft(); order.append(v)
            for x in self.out[v]:
                deg[x] -= 1
                if deg[x] == 0: q.append(x)
        if len(order) != n: raise AssertionError("the graph has a cycle")
        return order

    def label(self, v, c):
        """what adding base c aligned to node v does: the node reused, or ("new", smallest id of the sibling set)"""
        if self.letter[v] == c: return v
        for u in self.sib[v]:
            if self.letter[u] == c: return u
        return ("new", min(self.sib[v]))

    def add_sequence(self, s, w, outcome, counted=True):
        """s: bytes, w: per-base weights, outcome: {position: label} of the aligned bases; counted=False: a sequence that no coverage counts (the zero-weight
        backbone of a polishing window, polish_reference.py)"""
        prev = None
        for i, c in enumerate(s):
            lab = outcome.get(i)
            if lab is None: y = self.new_node(c)
            elif isinstance(lab, tuple): y = self.new_node(c, sibling_of=lab[1])
            else:
                y = lab; assert self.letter[y] == c
            if counted: self.count[y] += 1
            if prev is not None: self.add_edge(prev, y, int(w[i - 1]) + int(w[i]))
            prev = y


def score_matrix(G, s, mode, m, n, g, order, within=None):
    V, L = len(G.letter), len(s)
    sv = np.frombuffer(s, dtype=np.uint8)
    H = np.full((V, L + 1), NEG, dtype=np.int64)
    gj = g * np.arange(L + 1, dtype=np.int64)          # the virtual source row of GLOBAL / SEMI, and the offset of the left-move scan
    sc_of = {}
    a = np.empty(L + 1, dtype=np.int64)
    for v in order:
        if within is not None and v not in within: continue
        c = G.letter[v]
        if c not in sc_of: sc_of[c] = np.where(sv == c, m, n).astype(np.int64)
        sc = sc_of[c]
        preds = [u for u in G.inn[v] if within is None or u in within]
        pm = None
        if len(preds) == 1: pm = H[preds[0]]
        elif preds: pm = H[preds].max(axis=0)
        a[:] = NEG
        if mode == LOCAL:
            a[1:] = sc                                   # an alignment may start at any node: 0 + sc
            if pm is not None:
                np.maximum(a[1:], pm[:-1] + sc, out=a[1:]); np.maximum(a, pm + g, out=a)
            np.maximum(a, 0, out=a)
        elif mode == GLOBAL:
            base = pm if pm is not None else gj
            a[1:] = base[:-1] + sc; np.maximum(a, base + g, out=a)
        else:
            a[1:] = gj[:-1] + sc
            if pm is not None:
                np.maximum(a[1:], pm[:-1] + sc, out=a[1:]); np.maximum(a, pm + g, out=a)
        H[v] = gj + np.maximum.accumulate(a - gj)       # left moves: H[j] = max_k<=j (a[k] + (j - k) g)
    return H


def subgraph_nodes(G, a0, a1):
    """racon's sub-graph of a layer that spans the backbone positions [a0, a1] of a window graph whose FIRST sequence is the backbone (backbone position = node id):
    every node reached backwards - through in-edges and aligned siblings - from backbone node a1 without entering a backbone node below a0"""
    inside, stack = set(), [a1]
    while stack:
        v = stack.pop()
        if v in inside or v < a0: continue
        inside.add(v)
        stack.extend(G.inn[v]); stack.extend(G.sib[v])
    return inside


def align(G, s, mode, m, n, g, enumerate_all=True, within=None):
    """-> (outcome {position: label}, decided).  within (a set of nodes, polish_reference.py): the alignment sees those nodes only - edges from and to other
    nodes do not exist for it, so nodes without a predecessor / successor INSIDE are its sources / ends (GLOBAL to a sub-graph)"""
    V, L = len(G.letter), len(s)
    order = G.topo()
    H = score_matrix(G, s, mode, m, n, g, order, within)
    if mode == LOCAL:
        best = int(H.max())
        if best <= 0: return {}, True
        ends = [(int(v), int(j)) for v, j in np.argwhere(H == best)]
    else:
        inside = range(V) if within is None else sorted(within)
        cand = [v for v in inside if not any(within is None or x in within for x in G.out[v])] if mode == GLOBAL else list(inside)
        col = H[cand, L]; best = int(col.max())
        assert best > NEG // 2
        ends = [(cand[int(k)], L) for k in np.nonzero(col == best)[0]]
    if not enumerate_all: ends = ends[:1]
    chain = [None]; intern = {}                          # pairs so far as a hash-consed list: id -> (id of the rest, position, label)

    def cons(rest, pos, lab):
        key = (rest, pos, lab); r = intern.get(key)
        if r is None:
            r = len(chain); chain.append(key); intern[key] = r
        return r
    finals = []; seen = set(); stack = []
    for e in ends:
        st = (e[0], e[1], 0); seen.add(st); stack.append(st)
    branches = len(stack); over = False
    while stack:
        v, j, oid = stack.pop()
        h = int(H[v, j])
        if mode == LOCAL and h == 0:
            finals.append(oid); continue
        preds = G.inn[v] if within is None else [u for u in G.inn[v] if u in within]
        nxt = []; fin = []
        if j >= 1:
            scv = m if G.letter[v] == s[j - 1] else n
            o2 = None
            hit = [u for u in preds if int(H[u, j - 1]) + scv == h]
            src = (mode == LOCAL and scv == h) or (mode == GLOBAL and not preds and (j - 1) * g + scv == h) or (mode == SEMI and (j - 1) * g + scv == h)
            if hit or src:
                o2 = cons(oid, j - 1, G.label(v, s[j - 1]))
                for u in hit: nxt.append((u, j - 1, o2))
                if src: fin.append(o2)
        for u in preds:
            if int(H[u, j]) + g == h: nxt.append((u, j, oid))
        if mode == GLOBAL and not preds and j * g + g == h: fin.append(oid)
        if j >= 1 and int(H[v, j - 1]) + g == h: nxt.append((v, j - 1, oid))
        assert nxt or fin, "a traceback cell without a source"
        if not enumerate_all:
            if fin: fin, nxt = fin[:1], []
            else: nxt = nxt[:1]
        finals.extend(fin)
        new = 0
        for st in nxt:
            if st not in seen:
                seen.add(st); stack.append(st); new += 1
        branches += max(0, new + len(fin) - 1)
        if branches > PATH_CAP:
            over = True; break
    if over: return align(G, s, mode, m, n, g, enumerate_all=False, within=within)[0], False
    outs = set(finals)
    oid = finals[0]; outcome = {}
    while oid:
        oid, pos, lab = chain[oid]; outcome[pos] = lab
    return outcome, len(outs) == 1


def _relatives(G, start):
    """ancestors and descendants of a node"""
    anc, desc = set(), set()
    st = [start]
    while st:
        for u in G.inn[st.pop()]:
            if u not in anc: anc.add(u); st.append(u)
    st = [start]
    while st:
        for x in G.out[st.pop()]:
            if x not in desc: desc.add(x); st.append(x)
    return anc, desc


def _one_chain(G, nodes):
    """nodes (in topological order) form a simple chain: each one's only out-edge leads to the next, whose only in-edge it is"""
    return all(G.out[a] == [b] and list(G.inn[b]) == [a] for a, b in zip(nodes, nodes[1:]))


def heaviest_bundle(G, info=None, chain_ties=False):
    """-> (list of consensus nodes, decided); info (a dict) receives the number of branch completions.
    chain_ties (polish_reference.py; off = the behaviour of every other caller): a maximum score attained by several nodes is no tie when those nodes form one
    simple chain.  Zero-weight edges make that the rule in a polishing window whose layers stop short of the backbone's end: every backbone node behind the
    last supported one repeats its score.  Whichever of them takes over, the completion loop goes on from it to the same sink along the same edges - and a
    completion at a node whose successor has no other predecessor invalidates nothing and scores every node behind it as before - so the consensus is the same."""
    order = G.topo()
    V = len(order); score = [-1] * V; pred = [-1] * V
    decided = True

    def take(v, sc, pr, skip_invalid):
        """node v takes its best in-edge; returns True when two best in-edges tie in weight and predecessor score"""
        bk, bu, tie = None, -1, False
        for u, w in G.inn[v].items():
            if skip_invalid and sc[u] == -1: continue
            k = (w, sc[u])
            if bk is None or k > bk: bk, bu, tie = k, u, False
            elif k == bk: tie = True
        if bu < 0: sc[v], pr[v] = -1, -1
        else: sc[v], pr[v] = bk[0] + bk[1], bu
        return tie

    def walk(v, pr):
        path = []
        while v != -1: path.append(v); v = pr[v]
        return path[::-1]

    def complete(start, anc, desc, rescore_others):
        """spoa's branch completion with none / all of the nodes that are neither ancestors nor descendants of `start` scored again"""
        sc, pr = list(score), list(pred); tie = False
        for x in G.out[start]:
            for u in G.inn[x]:
                if u != start: sc[u] = -1
        cand = []
        for v in order:
            if v == start or v in anc or (v not in desc and not rescore_others): continue
            tie |= take(v, sc, pr, True); cand.append(v)
        top = max(sc[v] for v in cand)
        tied = [v for v in cand if sc[v] == top]
        tie |= len(tied) > 1 and not (chain_ties and _one_chain(G, tied))
        return sc, pr, next(v for v in cand if sc[v] == top), tie

    for v in order: decided &= not take(v, score, pred, False)
    top = max(score)
    tied = [v for v in order if score[v] == top]
    if len(tied) > 1 and not (chain_ties and _one_chain(G, tied)): decided = False
    mx = next(v for v in order if score[v] == top)
    while G.out[mx]:
        anc, desc = _relatives(G, mx)
        sa, pa, ma, ta = complete(mx, anc, desc, False)
        sb, pb, mb, tb = complete(mx, anc, desc, True)
        if ta or tb or ma != mb or walk(ma, pa) != walk(mb, pb): decided = False
        score, pred, mx = sa, pa, ma
        if info is not None: info["completions"] = info.get("completions", 0) + 1
    return walk(mx, pred), decided


def base_weights(n_bases, qual=None, weight=None):
    if weight is not None: return [min(max(int(weight), 1), WEIGHT_CAP)] * n_bases
    if qual is None: return [1] * n_bases
    q = qual.encode() if isinstance(qual, str) else bytes(qual)
    assert len(q) == n_bases
    return [c - 33 for c in q]


def poa_reference(seqs, quals=None, weights=None, mode=LOCAL, match=5, mismatch=-4, gap=-2, info=None):
    """one group -> (consensus string, uint32 coverage array, decided); info: see heaviest_bundle"""
    G = Graph(); decided = True
    for k, sq in enumerate(seqs):
        s = sq.encode() if isinstance(sq, str) else bytes(sq)
        if not s: continue
        w = base_weights(len(s), None if quals is None else quals[k], None if weights is None else weights[k])
        if not G.letter: outcome = {}
        else:
            outcome, ok = align(G, s, mode, match, mismatch, gap, enumerate_all=decided)
            decided = decided and ok
        G.add_sequence(s, w, outcome)
    if not G.letter: return "", np.zeros(0, dtype=np.uint32), True
    path, ok = heaviest_bundle(G, info)
    decided = decided and ok
    cons = bytes(G.letter[v] for v in path).decode()
    cov = np.array([sum(G.count[u] for u in G.sib[v]) for v in path], dtype=np.uint32)
    return cons, cov, decided
