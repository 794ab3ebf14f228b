"""The hot path end to end on one GPU: cluster -> draft consensus (spoa-style) -> rc merge -> polish (racon-style).

Array-level driver used by bench.py and by the reference-shaped host layer (cluster.py / consensus.py of this
package).  Everything heavy happens behind the C-ABI; this module only does the bookkeeping the reference does in
Python dicts, with numpy on index arrays.
"""
from __future__ import annotations
import time
import numpy as np
from ._capi import Api, ReadSet, cluster_params, poa_params, polish_params, POA_LOCAL

# Draft consensus: coverage-trim the ends of every tile consensus (ngsid_poa_params_t.trim).  spoa itself completes the heaviest bundle to
# a sink, so its consensus can end in the unsupported tail of a single read, and racon cannot shorten or extend a backbone end; with the
# trim the drafts of the noisy synthetic sets equal their amplicons before polishing.
# Reads per exact-order POA tile (draft and polishing windows).  With coverage-trimmed tile consensuses the depth does not matter for the accuracy on deep
# clusters (exact from 5.6 % to 14.3 % read error at depths 8 / 6 / 5 / 4: 0 of 250 polished sequences wrong per depth, 40 000 reads per cluster), and on shallow,
# noisy ones the SMALLER tile is the better one (100 reads per cluster at 14.3 % error: 12 of 100 polished sequences wrong at depth 4, 25 at depth 6; 200 reads and
# more: none at either) - profiles/r05_tile_depth_sweep.txt.  Round 5: 4 (was 6 since round 3): the graphs of a tile stay smaller (fewer rows per alignment), k_poa_tile
# 396 -> 363 ms per C3 step, the step 780 -> 748 ms; depth 3 loses the majority inside a tile (2 edits per amplicon on the bench workload) and is slower again.
TILE_DEPTH = 4
# Round 6: a unit (a cluster in the draft, a window in the polisher) with FEWER sequences than this is aligned as ONE graph in file order - spoa's / racon's own order
# (consensus.py:257-266,87) - instead of being tiled (ngsid_poa_params_t.single_below).  Tiling is a throughput device for deep clusters; profiles/r06_tile_depth_sweep.txt.
SINGLE_BELOW = 64
import os as _os
_TOUCH = bool(_os.environ.get("NGSID_TOUCH"))          # dev probe (round 5): one trivial device operation in the middle of the host work between clustering and consensus
DRAFT_TRIM = 1

_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTNacgtn", b"TGCANtgcan"):
    _COMP[_a] = _b


def revcomp_str(s: str) -> str:
    return _COMP[np.frombuffer(s.encode(), dtype=np.uint8)[::-1]].tobytes().decode()


def clusters_from_rep(rep_of: np.ndarray):
    """-> (reps, order, grp_off): clusters keyed by representative read; order lists each cluster's reads with the
    representative first and the members in processing order (cluster.py:338-345: the representative was processed
    before any read that joined it, and reads are processed in index order)."""
    from . import fastio
    return fastio.group_by_rep(rep_of)                               # three counting passes in the host library (NumPy: compare, cumsum, gather, radix argsort, bincount - 7 ms per 10^6 reads)


def select_centers(reps, counts, score, abundance_cutoff):
    """clusters sorted by (size, representative score) descending, size >= cutoff   (consensus.py:254-256)."""
    idx = np.lexsort((-score[reps], -counts))          # primary: size desc, secondary: score desc (stable)
    return [int(i) for i in idx if counts[i] >= abundance_cutoff]


def _rc_pairs(n, q0=0, t0=0, rc0=None):
    """(query, target) index lists of detect_reverse_complements for n centres: every i < j against j forward and j reverse-complemented.  The centres are
    q0 .. q0+n-1 of the query set, t0 .. of the target set, their reverse complements rc0 .. of the target set."""
    rc0 = n if rc0 is None else rc0
    qi, ti = [], []
    for i in range(n):
        for j in range(i + 1, n):
            qi += [q0 + i, q0 + i]; ti += [t0 + j, rc0 + j]
    return qi, ti


def _rc_decide(centers, ncols, nmatch, rc_identity_threshold):
    """the decision loop of consensus.detect_reverse_complements (consensus.py:163-183) on the alignment results of _rc_pairs(len(centers))"""
    n = len(centers)
    ident = {}
    p = 0
    for i in range(n):
        for j in range(i + 1, n):
            fw = nmatch[p] / float(ncols[p]); rc = nmatch[p + 1] / float(ncols[p + 1]); p += 2
            ident[(i, j)] = max(fw, rc)
    out, removed = [], set()
    for i in range(n):
        nr, cid, seq, groups = centers[i]
        if cid in removed:
            continue
        merged_n, allg = nr, list(groups)
        if i < n - 1:
            for j in range(i + 1, n):
                if ident[(i, j)] >= rc_identity_threshold:          # NB the reference also re-merges already removed centres
                    merged_n += centers[j][0]; removed.add(centers[j][1]); allg += list(centers[j][3])
        out.append([merged_n, cid, seq, allg])
    return out


def detect_reverse_complements(api: Api, centers, rc_identity_threshold):
    """consensus.detect_reverse_complements (consensus.py:148-183): centers = [n_reads, c_id, seq, groups(list of cluster ids)].
    Identity = matching columns / alignment columns of the semi-global alignment (open 3, ext 1, +2/-2), max over fw / rc."""
    return detect_reverse_complements_samples(api, [centers], rc_identity_threshold)[0]


def detect_reverse_complements_samples(api: Api, centers_per_sample, rc_identity_threshold):
    """detect_reverse_complements for several samples with ONE alignment call: pairs only within a sample, the decision loop per sample"""
    seqs = [c[2] for cs in centers_per_sample for c in cs]
    nall = len(seqs)
    qi, ti, span = [], [], []
    base = 0
    for cs in centers_per_sample:
        n = len(cs)
        a, b = (_rc_pairs(n, base, base, nall + base) if n > 1 else ([], []))
        span.append((len(qi), len(qi) + len(a))); qi += a; ti += b
        base += n
    ncols = nmatch = None
    if qi:
        q = ReadSet.from_strings(seqs); t = ReadSet.from_strings(seqs + [revcomp_str(s) for s in seqs])
        _, ncols, nmatch, _ = api.sg_align_batch(q, t, qi, ti, 3, 1, 2, -2, 13, None)
    out = []
    for cs, (a, b) in zip(centers_per_sample, span):
        out.append([[c[0], c[1], c[2], list(c[3])] for c in cs] if len(cs) <= 1 else _rc_decide(cs, ncols[a:b], nmatch[a:b], rc_identity_threshold))
    return out


def pooled_read_lists(merged, group_reads):
    """reads polished against every merged centre: the pooled files of consensus.py:208-215.  The reference re-merges centres that were removed
    already (detect_reverse_complements above), so one cluster can be pooled under two centres; the polisher keeps strand and layers per read, so
    a read stays with the FIRST centre that lists it (a deviation in that rare case, logged)."""
    seen = set(); out = []; dup = 0
    for m in merged:
        parts = []
        for ci in m[3]:
            if ci in seen:
                dup += 1; continue
            seen.add(ci); parts.append(group_reads(ci))
        out.append(np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32))
    if dup:
        import logging
        logging.warning("%d cluster(s) were merged into more than one centre: their reads polish the first of them only", dup)
    return out


def group_offsets(lists):
    """group offsets of the concatenation of lists: [0, len(lists[0]), len(lists[0]) + len(lists[1]), ...]"""
    return np.concatenate(([0], np.cumsum([len(x) for x in lists])))


def _deal(flat, sizes):
    """a flat list of results cut back into consecutive runs of sizes[0], sizes[1], ... entries"""
    out, x = [], 0
    for n in sizes:
        out.append(flat[x:x + n]); x += n
    return out


def _support_of(api, rs, seqs, lists, k, w):
    """Api.consensus_support of the sequences seqs over their read lists, ONE call -> one [len, 8] array per sequence"""
    if not seqs:
        return []
    counts, cen_off, _, _ = api.consensus_support(ReadSet.from_strings(seqs), rs, group_offsets(lists), read_order=np.concatenate(lists), k=k, w=w)
    return [counts[int(cen_off[i]):int(cen_off[i + 1])] for i in range(len(seqs))]


def _consensus_stages(api, rs, score, seg_off, out, bands, T, k, w, abundance_ratio, rc_identity_threshold, max_seqs_for_consensus, racon_iter, tile_depth, node_cap,
                      do_polish, polish_trim, polish_aln_mode, polish_stop_when_stable, draft_trim, single_below, support, classify, classify_kwargs, chimeras=False, chimera_kwargs=None, hp_polish=False, hp_kwargs=None, recruit=False, recruit_kwargs=None, alignments=False, alignment_kwargs=None, error_profile=False, error_profile_kwargs=None):
    """Everything behind the clustering call, once for a list of samples: reads [seg_off[s], seg_off[s+1]) of rs are sample s, out[s] is its result dict (rep_of in read
    indices local to the sample) and bands[s] the band of its draft and polishing calls.  Per sample the cluster table and the selection with the sample's own cut-off, the
    reverse-complement bookkeeping and the pooled read lists; for all samples ONE alignment call, one consensus_support call and one search, and per distinct band one draft
    and one polishing call.  Fills centers (and support / classify, when asked for) into the dicts of the samples that have a centre above their cut-off and leaves the other
    dicts as they are.  hp_polish (extension, hp.py): the homopolymer run-length vote over the final sequences of ALL samples - one Api.hp_runs call per round - after
    the polishing (or the draft, without it) and before support, classification and chimeras, which see the corrected sequences; hp_polish of a sample's dict = one change
    table per centre.  error_profile (extension, errprof.py): the read error tables of the final sequences over the lists of support, one Api.error_profile call for all
    samples.  -> None when no sample has one, else (polished, pooled, prms): polished[s] the final sequences and pooled[s] the polisher's read lists (read numbers
    of rs) of every centre of sample s, prms[band] the (draft, polish or None) parameter structs of that band's calls."""
    tile_depth = TILE_DEPTH if tile_depth is None else tile_depth
    single_below = SINGLE_BELOW if single_below is None else single_below
    # ---- per-sample cluster tables and selections
    t0 = time.perf_counter()
    tab = {}                                                                    # the samples with a centre: s -> (reps, order, grp_off, counts, sel), order in read numbers of rs
    for s, o in enumerate(out):
        a0, n = int(seg_off[s]), int(seg_off[s + 1]) - int(seg_off[s])
        if n == 0:
            continue
        reps, order, grp_off, counts = clusters_from_rep(o["rep_of"])
        sel = select_centers(reps, counts, score[a0:a0 + n], int(abundance_ratio * n))      # NGSpeciesID:65, per sample
        if sel:
            tab[s] = (reps, (order + np.uint32(a0)) if a0 else order, grp_off, counts, sel)  # (a sample that starts at read 0 is not copied: a million indices per step in bench.py)
    if _TOUCH and hasattr(api, "ctx"):
        import ctypes as _C
        api.lib.ngsid_ctx_option(api.ctx, b"touch", _C.c_int64(1))
    T["host_group"] = T.get("host_group", 0.0) + time.perf_counter() - t0
    if not tab:
        return None
    def cluster_reads(s, ci):                                                   # the reads of cluster ci of sample s that the consensus stages see
        _, order, grp_off = tab[s][:3]
        a, b = int(grp_off[ci]), int(grp_off[ci + 1])
        if max_seqs_for_consensus >= 0:
            b = min(b, a + max_seqs_for_consensus)                              # consensus.py:260; the pooled file is built from the truncated reads_c_id files too
        return order[a:b]
    by_band = {bnd: [s for s in tab if bands[s] == bnd] for bnd in sorted({bands[s] for s in tab})}      # the samples that share their draft and polishing calls
    # ---- draft consensus: one call per band
    t0 = time.perf_counter()
    drafts, prms = {}, {}
    for bnd, ss in by_band.items():
        keys = [(s, ci) for s in ss for ci in tab[s][4]]
        parts = [cluster_reads(s, ci) for s, ci in keys]
        prms[bnd] = [poa_params(mode=POA_LOCAL, match=5, mismatch=-4, gap=-2, tile_depth=tile_depth, band=bnd, node_cap=node_cap, trim=DRAFT_TRIM if draft_trim is None else draft_trim, single_below=single_below), None]
        drafts.update(zip(keys, api.poa_consensus(rs, group_offsets(parts), prms[bnd][0], read_order=np.concatenate(parts))))
    T["consensus"] = T.get("consensus", 0.0) + time.perf_counter() - t0
    # ---- reverse-complement detection: one alignment call, pairs within a sample only
    t0 = time.perf_counter()
    centers = [[[int(tab[s][3][ci]), int(tab[s][0][ci]), drafts[(s, ci)], [ci]] for ci in tab[s][4]] for s in tab]
    merged = dict(zip(tab, detect_reverse_complements_samples(api, centers, rc_identity_threshold)))
    T["rc_merge"] = T.get("rc_merge", 0.0) + time.perf_counter() - t0
    # ---- pooled read lists (consensus.py:208-215) and polishing: one call per band
    t0 = time.perf_counter()
    pooled = {s: pooled_read_lists(merged[s], lambda ci, s=s: cluster_reads(s, ci)) for s in tab}
    polished = {s: [m[2] for m in merged[s]] for s in tab}
    if do_polish and racon_iter > 0:
        for bnd, ss in by_band.items():
            lists = [l for s in ss for l in pooled[s]]
            prms[bnd][1] = polish_params(iters=racon_iter, k=k, w=w, tile_depth=tile_depth, band=bnd, node_cap=node_cap, trim=polish_trim, aln_mode=polish_aln_mode, stop_when_stable=polish_stop_when_stable, single_below=single_below)
            pol, _ = api.polish(ReadSet.from_strings([m[2] for s in ss for m in merged[s]]), rs, group_offsets(lists), prms[bnd][1], read_order=np.concatenate(lists))      # (dealt to two contexts when it pays: _capi.Api lanes)
            polished.update(zip(ss, _deal(pol, [len(merged[s]) for s in ss])))
        T["polish"] = T.get("polish", 0.0) + time.perf_counter() - t0
    if hp_polish:
        from . import hp as hp_mod
        t0 = time.perf_counter()
        sizes = [len(merged[s]) for s in tab]
        new, changes = hp_mod.polish(api, [q for s in tab for q in polished[s]], rs, [l for s in tab for l in pooled[s]], k=k, w=w, **(hp_kwargs or {}))
        for s, seqs_, ch in zip(tab, _deal(new, sizes), _deal(changes, sizes)):
            polished[s] = list(seqs_); out[s]["hp_polish"] = ch
        T["hp_polish"] = T.get("hp_polish", 0.0) + time.perf_counter() - t0
    for s in tab:
        reps = tab[s][0]
        out[s]["centers"] = [(m[0], m[1], m[2], polished[s][i], [int(reps[ci]) for ci in m[3]]) for i, m in enumerate(merged[s])]
    # ---- read support and classification of the final sequences: one call each
    flat = [q for s in tab for q in polished[s]]; sizes = [len(merged[s]) for s in tab]
    if support:
        t0 = time.perf_counter()
        for s, part in zip(tab, _deal(_support_of(api, rs, flat, [l for s in tab for l in pooled[s]], k, w), sizes)):
            out[s]["support"] = part
        T["support"] = T.get("support", 0.0) + time.perf_counter() - t0
    if error_profile:                                                           # the read error tables of the final sequences over the lists support=True takes: one call
        from . import errprof as errprof_mod
        t0 = time.perf_counter()
        for s, part in zip(tab, _deal(errprof_mod.profile(api, rs, flat, [l for s in tab for l in pooled[s]], k=k, w=w, **(error_profile_kwargs or {})), sizes)):
            out[s]["error_profile"] = part
        T["error_profile"] = T.get("error_profile", 0.0) + time.perf_counter() - t0
    if classify is not None:
        from . import classify as classify_mod
        t0 = time.perf_counter()
        for s, part in zip(tab, _deal(classify_mod.identify(api, classify, flat, **(classify_kwargs or {})), sizes)):
            out[s]["classify"] = part
        T["classify"] = T.get("classify", 0.0) + time.perf_counter() - t0
    if chimeras:
        from . import chimera as chimera_mod
        t0 = time.perf_counter()
        per = chimera_mod.detect(api, flat, [m[0] for s in tab for m in merged[s]], np.concatenate(([0], np.cumsum(sizes))), **(chimera_kwargs or {}))
        for s, part in zip(tab, per):
            out[s]["chimeras"] = part
        T["chimeras"] = T.get("chimeras", 0.0) + time.perf_counter() - t0
    if recruit:
        from . import recruit as recruit_mod
        t0 = time.perf_counter()
        ns = len(out)
        origins = [None] * ns
        for s in tab:                                                           # the centre whose pooled clusters hold a read: whole clusters, the first centre that lists one
            a0, n = int(seg_off[s]), int(seg_off[s + 1]) - int(seg_off[s])
            order, grp_off = tab[s][1], tab[s][2]
            lists = [np.concatenate([order[int(grp_off[ci]):int(grp_off[ci + 1])].astype(np.int64) - a0 for ci in m[3]]) for m in merged[s]]
            origins[s] = recruit_mod.origin_of(n, lists)
        per = recruit_mod.run(api, rs, np.asarray(seg_off, dtype=np.int64), [list(polished[s]) if s in tab else [] for s in range(ns)], origins,
                              [[m[0] for m in merged[s]] if s in tab else None for s in range(ns)], **(recruit_kwargs or {}))
        for o, part in zip(out, per):
            o["recruit"] = part
        T["recruit"] = T.get("recruit", 0.0) + time.perf_counter() - t0
    if alignments:
        from . import sam as sam_mod
        t0 = time.perf_counter()
        lists = {}                                                              # per sample the reads listed under every centre, read numbers of rs
        for s in tab:
            if recruit:                                                         # every assigned read under its recruited centre (sam.recruited_lists)
                a0 = np.uint32(int(seg_off[s]))
                lists[s] = [l + a0 for l in sam_mod.recruited_lists(out[s]["recruit"]["hits"], out[s]["recruit"]["status"], len(polished[s]))[0]]
            else:
                lists[s] = [np.asarray(l, dtype=np.uint32) for l in pooled[s]]
        parts = sam_mod.align(api, rs, flat, [l for s in tab for l in lists[s]], k=k, w=w, **(alignment_kwargs or {}))
        for s, part in zip(tab, _deal(parts, sizes)):
            a0 = int(seg_off[s])
            for e in part: e["reads"] = e["reads"].astype(np.int64) - a0         # local to the sample, like rep_of
            out[s]["alignments"] = part
        T["alignments"] = T.get("alignments", 0.0) + time.perf_counter() - t0
    return polished, pooled, prms


def run_hot_path(api: Api, rs: ReadSet, score: np.ndarray, acc_rank=None, k=13, w=20, abundance_ratio=0.1,
                 rc_identity_threshold=0.9, max_seqs_for_consensus=-1, racon_iter=3, tile_depth=None, band=0, node_cap=0,
                 p_shared=None, cluster_kwargs=None, do_consensus=True, do_polish=True, timings=None, polish_trim=2, polish_aln_mode=2, polish_stop_when_stable=True,
                 strand_aware=False, draft_trim=None, single_below=None, support=False, classify=None, classify_kwargs=None, split_haplotypes=False, haplotype_kwargs=None, chimeras=False, chimera_kwargs=None,
                 hp_polish=False, hp_kwargs=None, recruit=False, recruit_kwargs=None, alignments=False, alignment_kwargs=None, error_profile=False, error_profile_kwargs=None):
    """Returns dict(rep_of, status, counters, hpc_err, centers=[(n_reads, c_id, draft, polished, groups)]); with strand_aware (extension, off by
    default: strand.py) also flip [n] = reads that were reverse-complemented for the consensus stages, and rep_of is the merged membership.
    support=True (extension): also support = one [len, 8] uint32 array per centre - the read support of every base of its final sequence over the pooled reads the
    polisher takes (Api.consensus_support); every other key is what support=False returns.
    classify=RefDb (extension; Api.refdb_build): also classify = one list of ranked hits per centre (classify.identify: its final sequence searched in the reference
    library and verified by alignment; classify_kwargs: top_k, min_shared, min_identity, min_query_cov); every other key is what classify=None returns.
    split_haplotypes=True (extension; phase.py, include/ngsid_phase.h): also haplotypes = one entry per centre, None or dict(sites, alleles [H, S], n_reads [H], assign
    [per pooled read] int8, draft [H], polished [H], used [H] and, with classify, classify [H]): the centre's pooled reads split by linked variant sites of its final sequence, every
    haplotype drafted and polished with the parameters of the cluster's own draft and polish (haplotype_kwargs: the policy arguments of phase.split_many); every other key
    is what split_haplotypes=False returns.
    chimeras=True (extension; chimera.py, include/ngsid_chimera.h): also chimeras = one dict per centre (chimera.describe: chimeric, the best single parent, the best
    two-parent model and its breakpoint interval, parents as centre numbers) - every centre's final sequence modelled from the more abundant centres, both strands
    (chimera_kwargs: min_abskew, min_gain, max_model_frac); every other key is what chimeras=False returns.
    hp_polish=True (extension; hp.py, include/ngsid_hp.h): the homopolymer finishing pass - a run-length vote of the pooled reads over every run of every final sequence, not
    a neural polisher - rewrites centers[..][3] before support, classification, chimeras and haplotypes see it; also hp_polish = one list per centre of
    dict(round, pos, letter, old, new, hist [2, 17]) for the runs it changed (hp_kwargs: rounds and the thresholds of hp.call).
    recruit=True (extension; recruit.py, include/ngsid_recruit.h): also recruit = dict(hits [n, 6] int32 in RECRUIT_FIELDS order with centre numbers, status [n] int8, counts =
    recruit.recount): every read of the call (the oriented ones under strand_aware) located inside every final sequence on both strands, ONE Api.recruit call behind hp_polish
    (recruit_kwargs: min_identity, q, min_margin, both_strands); every other key is what recruit=False returns.
    alignments=True (extension; sam.py, include/ngsid_cigar.h): also alignments = one dict(reads, strand, aln [n, 5] in CIGAR_FIELDS order, op_off, ops) per centre - the
    alignment of every listed read to the centre's final sequence, ONE Api.read_cigars call behind hp_polish; the reads listed are the pooled lists the polisher takes, with
    recruit=True every assigned read under its recruited centre (alignment_kwargs: clip, merge_m, cap); every other key is what alignments=False returns.
    error_profile=True (extension; errprof.py, include/ngsid_errprof.h): also error_profile = one dict(counts [2, 96], qtab [2, 94, 3] or None, n_listed, n_stranded) per centre -
    what the pooled reads the polisher takes (the lists of support=True) did to the letters of the centre's final sequence, ONE Api.error_profile call behind hp_polish
    (error_profile_kwargs: clip, qualities); every other key is what error_profile=False returns.  The centre is made of the same reads: errprof.py says what that hides."""
    T = timings if timings is not None else {}
    t0 = time.perf_counter()
    prm = cluster_params(k=k, w=w, p_shared=p_shared, **(cluster_kwargs or {}))
    rep_of, herr, status, counters = api.cluster_greedy(rs, prm, acc_rank=acc_rank)
    T["cluster"] = T.get("cluster", 0.0) + time.perf_counter() - t0
    res = dict(rep_of=rep_of, status=status, counters=counters, hpc_err=herr, centers=[])
    n = rs.n
    if strand_aware:
        from . import strand
        t0 = time.perf_counter()
        rep_of, flip, _, sinfo = strand.strand_merge(api, rs, rep_of, score, prm, min_size=max(2, int(abundance_ratio * n) // 2))
        if flip.any():
            rs = strand.orient_reads(rs, flip)                                   # the consensus stages see every cluster in one orientation
        res.update(rep_of=rep_of, flip=flip, strand_info=sinfo)
        T["strand_merge"] = T.get("strand_merge", 0.0) + time.perf_counter() - t0
    if classify is not None: res["classify"] = []                               # what stays without a centre: nothing to name, nothing to split
    if split_haplotypes: res["haplotypes"] = []
    if chimeras: res["chimeras"] = []
    if hp_polish: res["hp_polish"] = []
    if recruit:
        from . import recruit as recruit_mod
        res["recruit"] = recruit_mod.nothing(n)                                  # what stays without a centre: every read unassigned
    if alignments: res["alignments"] = []
    if error_profile: res["error_profile"] = []
    if not do_consensus:
        return res
    # one sample, reads [0, n); band goes through as it is: for band <= 0 the library applies the POA_BAND64_MAXLEN rule to the reads of the call, which here are the sample's
    # (reading the lengths of a device-resident set here would cost a copy of its offsets to the host in every step)
    stages = _consensus_stages(api, rs, score, [0, n], [res], [band], T, k, w, abundance_ratio, rc_identity_threshold, max_seqs_for_consensus, racon_iter, tile_depth, node_cap,
                               do_polish, polish_trim, polish_aln_mode, polish_stop_when_stable, draft_trim, single_below, support, classify, classify_kwargs, chimeras, chimera_kwargs, hp_polish, hp_kwargs,
                               recruit, recruit_kwargs, alignments, alignment_kwargs, error_profile, error_profile_kwargs)
    if split_haplotypes and stages is not None:
        from . import phase
        t0 = time.perf_counter()
        polished, pooled, prms = stages
        haps = phase.build(api, rs, list(polished[0]), pooled[0], *prms[band], supports=res.get("support"), k=k, w=w, **(haplotype_kwargs or {}))
        if classify is not None:
            from . import classify as classify_mod
            seqs = [q for e in haps if e is not None for q in e["polished"]]
            hits = classify_mod.identify(api, classify, seqs, **(classify_kwargs or {})) if seqs else []
            for e, part in zip(haps, _deal(hits, [0 if e is None else len(e["polished"]) for e in haps])):
                if e is not None: e["classify"] = part
        res["haplotypes"] = haps
        T["haplotypes"] = T.get("haplotypes", 0.0) + time.perf_counter() - t0
    return res


POA_BAND64_MAXLEN = 3000       # include/ngsid.h NGSID_POA_BAND64_MAXLEN: band <= 0 means 64 columns iff every read of the call has at most this many bases, else 128


def _bands_alone(rs, so, band):
    """the band every sample [so[s], so[s+1]) of rs gets when it is run alone: band when it is given, else the library's rule for band <= 0 on the sample's own reads"""
    if band > 0:
        return [band] * (len(so) - 1)
    if rs.mem == 0:
        lens = np.diff(rs.off.astype(np.int64))
    else:
        kp = rs.keep if isinstance(rs.keep, dict) else {}
        lens = np.diff(kp["host"].off.astype(np.int64)) if kp.get("host") is not None else np.diff(kp["off"].cpu().numpy().astype(np.int64))
    return [64 if a == b or int(lens[a:b].max()) <= POA_BAND64_MAXLEN else 128 for a, b in zip(so[:-1], so[1:])]


def run_hot_path_samples(api: Api, rs: ReadSet, score: np.ndarray, seg_off, acc_rank=None, k=13, w=20, abundance_ratio=0.1,
                         rc_identity_threshold=0.9, max_seqs_for_consensus=-1, racon_iter=3, tile_depth=None, band=0, node_cap=0,
                         p_shared=None, cluster_kwargs=None, do_consensus=True, do_polish=True, timings=None, polish_trim=2, polish_aln_mode=2, polish_stop_when_stable=True,
                         strand_aware=False, draft_trim=None, single_below=None, support=False, classify=None, classify_kwargs=None, chimeras=False, chimera_kwargs=None,
                         variants=False, variant_kwargs=None, hp_polish=False, hp_kwargs=None, recruit=False, recruit_kwargs=None, alignments=False, alignment_kwargs=None,
                         error_profile=False, error_profile_kwargs=None):
    """run_hot_path for many samples in one pass: reads [seg_off[s], seg_off[s+1]) of rs (each sample in its own score order) are sample s.  Returns one
    run_hot_path-shaped dict per sample, read indices local to the sample - what run_hot_path returns for that sample's reads alone.  One segmented clustering
    call, one draft consensus call, one alignment call for the reverse-complement detection and one polishing call serve all samples; with band <= 0 the samples
    are grouped by the band they would get alone (a sample with a read above POA_BAND64_MAXLEN bases gets 128 columns, the others 64), so at most two consensus
    and two polishing calls.  support=True: the support key of run_hot_path per sample, from one consensus_support call for all samples.  classify=RefDb: the classify
    key of run_hot_path per sample, the final consensuses of ALL samples in one search and one verification call.  chimeras=True: the chimeras
    key of run_hot_path per sample, ALL samples in one model call (parents within a sample only).  variants=True (extension; variants.py, include/ngsid_near.h):
    also variants = dict(members = one dict(variant, dist, strand) per centre of the sample, table = the study-wide table of variants.build, the same object in every
    sample's dict): the final sequences of ALL samples in one near-pairs call, clustered by abundance (variant_kwargs: identity, max_dist, both_strands, wide_max_dist - the last replaces max_dist and takes the wide kernels); every other key
    is what variants=False returns.  hp_polish=True: the hp_polish key of run_hot_path per sample, ONE Api.hp_runs call per round for all samples; the variants see the
    corrected sequences.  recruit=True: the recruit key of run_hot_path per sample (read indices and centre numbers local to the sample), ONE Api.recruit call for all
    samples.  alignments=True: the alignments key of run_hot_path per sample (read indices local to the sample), ONE Api.read_cigars call for all samples.
    error_profile=True: the error_profile key of run_hot_path per sample, ONE Api.error_profile call for all samples.
    strand_aware is not supported here (ValueError)."""
    if strand_aware:
        raise ValueError("run_hot_path_samples: strand_aware is not supported in multi-sample mode (run the samples one by one)")
    T = timings if timings is not None else {}
    so = np.asarray(seg_off, dtype=np.int64); ns = len(so) - 1
    t0 = time.perf_counter()
    prm = cluster_params(k=k, w=w, p_shared=p_shared, **(cluster_kwargs or {}))
    rep_of, herr, status, counters = api.cluster_greedy_segmented(rs, prm, so.astype(np.uint64), acc_rank=acc_rank)
    T["cluster"] = T.get("cluster", 0.0) + time.perf_counter() - t0
    out = [dict(rep_of=rep_of[so[s]:so[s + 1]] - np.int32(so[s]), status=status[so[s]:so[s + 1]], counters=counters[s], hpc_err=herr[so[s]:so[s + 1]], centers=[]) for s in range(ns)]
    if classify is not None:
        for o in out: o["classify"] = []                                        # what stays for a sample without a centre
    if chimeras:
        for o in out: o["chimeras"] = []
    if variants:
        for o in out: o["variants"] = None
    if hp_polish:
        for o in out: o["hp_polish"] = []
    if recruit:
        from . import recruit as recruit_mod
        for s, o in enumerate(out): o["recruit"] = recruit_mod.nothing(int(so[s + 1] - so[s]))
    if alignments:
        for o in out: o["alignments"] = []
    if error_profile:
        for o in out: o["error_profile"] = []
    if not do_consensus:
        return out
    t0 = time.perf_counter()
    bands = _bands_alone(rs, so, band)
    T["host_group"] = T.get("host_group", 0.0) + time.perf_counter() - t0
    _consensus_stages(api, rs, score, so, out, bands, T, k, w, abundance_ratio, rc_identity_threshold, max_seqs_for_consensus, racon_iter, tile_depth, node_cap,
                      do_polish, polish_trim, polish_aln_mode, polish_stop_when_stable, draft_trim, single_below, support, classify, classify_kwargs, chimeras, chimera_kwargs, hp_polish, hp_kwargs,
                      recruit, recruit_kwargs, alignments, alignment_kwargs, error_profile, error_profile_kwargs)
    if variants:
        from . import variants as variants_mod
        t0 = time.perf_counter()
        tab = variants_mod.build(api, variants_mod.collect([(s, None, [(c[1], c[0], c[3]) for c in o["centers"]]) for s, o in enumerate(out)]), **(variant_kwargs or {}))
        at = 0
        for o in out:
            n = len(o["centers"])
            o["variants"] = dict(members=[dict(variant=int(tab["variant_of"][x]), dist=int(tab["dist"][x]), strand=int(tab["strand"][x])) for x in range(at, at + n)], table=tab)
            at += n
        T["variants"] = T.get("variants", 0.0) + time.perf_counter() - t0
    return out
