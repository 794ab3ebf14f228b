"""Reference of ngsid_classify_search, written from include/ngsid_classify.h.  Test infrastructure - never imported by the product.

It shares one thing with the library: the minimizer call.  Codes come from Api.hpc_minimizers of whichever backend is handed in (the CPU oracle, or the library on
the GPU); reverse complements are built in numpy, the code sets are Python sets, |S(q_s) & S(r)| is a set intersection, and the reduction over strands, the
min_shared filter and the (shared descending, ref ascending) order are numpy.  Also: a generator of libraries and queries with known truth.
"""
import numpy as np
from ngspeciesid_amd._capi import ReadSet

_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


def revcomp(s: str) -> str:
    return _COMP[np.frombuffer(s.encode(), dtype=np.uint8)[::-1]].tobytes().decode()


def code_sets(api, seqs, k, w):
    """S(x) for every sequence: the distinct codes of Api.hpc_minimizers (qualities are a constant: they never influence a code)"""
    seqs = list(seqs)
    if not seqs:
        return []
    moff, codes, _, _, _ = api.hpc_minimizers(ReadSet.from_strings(seqs, ["I" * len(s) for s in seqs]), k, w)
    return [set(codes[int(moff[i]):int(moff[i + 1])].tolist()) for i in range(len(seqs))]


def shared_counts(ref_sets, fwd_sets, rc_sets):
    """-> shared [n_queries, 2, n_refs] int32"""
    out = np.zeros((len(fwd_sets), 2, len(ref_sets)), dtype=np.int32)
    for q, pair in enumerate(zip(fwd_sets, rc_sets)):
        for s, qs in enumerate(pair):
            if qs:
                out[q, s] = [len(qs & r) for r in ref_sets]
    return out


def select(shared, top_k, min_shared):
    """shared [n, 2, R] -> (cand_ref, cand_shared [n, top_k] int32, cand_strand [n, top_k] int8), -1 where a query has fewer candidates"""
    n, _, R = shared.shape
    ref = np.full((n, top_k), -1, dtype=np.int32); sh = np.full((n, top_k), -1, dtype=np.int32); st = np.full((n, top_k), -1, dtype=np.int8)
    best = shared.max(axis=1); strand = (shared[:, 1] > shared[:, 0]).astype(np.int8)          # strand 0 on a tie
    idx = np.arange(R)
    for q in range(n):
        order = np.lexsort((idx, -best[q].astype(np.int64)))                                  # shared descending, then ref ascending
        order = order[best[q][order] >= min_shared][:top_k]
        m = len(order)
        ref[q, :m] = order; sh[q, :m] = best[q][order]; st[q, :m] = strand[q][order]
    return ref, sh, st


def search(api, refs, queries, k, w, top_k, min_shared, ref_sets=None):
    """the four arrays of Api.classify_search(..., n_codes=True)"""
    refs, queries = list(refs), list(queries)
    rsets = code_sets(api, refs, k, w) if ref_sets is None else ref_sets
    f, r = code_sets(api, queries, k, w), code_sets(api, [revcomp(q) for q in queries], k, w)
    ncodes = np.array([[len(a), len(b)] for a, b in zip(f, r)], dtype=np.int32).reshape(len(queries), 2)
    return select(shared_counts(rsets, f, r), top_k, min_shared) + (ncodes,)


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def mutate(rng, s, rate):
    """substitutions and indels at `rate` per base: a third each"""
    out = []
    for ch in s:
        u = rng.random()
        if u < rate / 3: out.append("ACGT"[("ACGT".index(ch) + int(rng.integers(1, 4))) % 4] if ch in "ACGT" else "A")
        elif u < 2 * rate / 3: pass
        elif u < rate: out.append(ch); out.append("ACGT"[int(rng.integers(0, 4))])
        else: out.append(ch)
    return "".join(out)


def make_truth(seed, n_members=200, length=400, divergence=0.15, n_queries=60, rate=0.03):
    """a library of n_members species of synth.make_species (pairwise related through their root) and n_queries queries, each a mutated copy (`rate`: substitutions
    and indels) of a known member, every third one reverse-complemented -> dict(refs, queries, member [n_queries], strand [n_queries])"""
    from ngspeciesid_amd import synth
    refs = [a.tobytes().decode() for a in synth.make_species(n_members, length, divergence, seed=seed)]
    rng = np.random.default_rng(seed + 77)
    member = rng.integers(0, n_members, n_queries); strand = (np.arange(n_queries) % 3 == 2).astype(np.int8)
    queries = []
    for m, s in zip(member.tolist(), strand.tolist()):
        q = mutate(rng, refs[m], rate)
        queries.append(revcomp(q) if s else q)
    return dict(refs=refs, queries=queries, member=member.astype(np.int32), strand=strand)
