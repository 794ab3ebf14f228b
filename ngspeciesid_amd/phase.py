"""Splitting a cluster into haplotypes by linked variant sites (extension; `--split_haplotypes`, `pipeline.run_hot_path(split_haplotypes=True)`): the policy on top of
ngsid_phase_genotypes / ngsid_phase_pair_tables / ngsid_phase_assign (include/ngsid_phase.h, csrc/k_phase.hip).

The device calls answer three questions with integers: which allele does every read carry at chosen centre positions, how often do the alleles of two positions occur
together, and which of a set of allele strings is every read nearest to.  Everything that is a choice lives here, in numpy, deterministic and without device work: which
positions are candidate sites (from the support counters), which of them are real (linked to another site - a systematic homopolymer error reaches 10 - 20 % at one column but
is independent between columns), which allele strings are haplotypes (by default only strings over each site's two most frequent alleles, the ones the linkage test looked at: `top2_only`), and how clear an
assignment has to be.  The defaults were settled on the CPU reference over synthetic
sets: profiles/phase.txt."""
from __future__ import annotations
import numpy as np
from ._capi import ReadSet, MEM_HOST, PHASE_MAX_SITES, PHASE_MAX_HAPS, GENO_DEL, HAP_ANY, phase_offsets

DEFAULTS = dict(min_alt_frac=0.15, min_alt_reads=5, min_phi=0.5, single_min_frac=0.25, min_hap_reads=10, min_hap_frac=0.05, max_haps=8, min_margin=1, top2_only=True)
ALLELES = "ACGT-"
_EPS = 1e-9           # ceil(f * n) <= c for an integer c is f * n - _EPS <= c: keeps 0.15 * 100 = 15.000000000000002 from asking for 16


def allele_counts(counts, centre):
    """[len, 5] allele counts A C G T del of every base from the [len, 8] support counters: the centre's own base gets `agree`, the others their `sub_*`"""
    c = np.asarray(counts).reshape(-1, 8).astype(np.int64)
    al = np.concatenate((c[:, 2:6], c[:, 6:7]), axis=1)
    code = np.full(256, 4, dtype=np.int64)
    for i, ch in enumerate(b"ACGT"): code[ch] = i; code[ch + 32] = i
    cb = code[np.frombuffer(centre.encode(), dtype=np.uint8)] if isinstance(centre, str) else code[np.asarray(centre, dtype=np.uint8)]
    if len(cb) != len(al): raise ValueError("support table of %d rows for a centre of %d bases" % (len(al), len(cb)))
    base = np.nonzero(cb < 4)[0]
    al[base, cb[base]] += c[base, 1]
    return al


def candidate_sites(counts, centre, min_alt_frac=DEFAULTS["min_alt_frac"], min_alt_reads=DEFAULTS["min_alt_reads"], max_sites=PHASE_MAX_SITES):
    """positions (ascending, uint32) whose second-largest allele count is at least max(min_alt_reads, ceil(min_alt_frac * depth)); more than max_sites of them: the ones
    with the largest second count, the lower position on ties"""
    c = np.asarray(counts).reshape(-1, 8)
    second = np.sort(allele_counts(c, centre), axis=1)[:, -2]
    need = np.maximum(float(min_alt_reads), min_alt_frac * c[:, 0].astype(np.float64) - _EPS)
    pos = np.nonzero(second >= need)[0]
    if len(pos) > max_sites:
        pos = np.sort(pos[np.lexsort((pos, -second[pos]))][:max_sites])
    return pos.astype(np.uint32)


def _top2(m):
    """the two most frequent codes of a marginal, the lower code on ties"""
    o = np.argsort(-np.asarray(m, dtype=np.int64), kind="stable")
    return int(o[0]), int(o[1])


def pair_phi(table):
    """phi coefficient of a 5 x 5 pair table reduced to the two most frequent alleles of each site (by the table's marginals); 0 when a marginal of the 2 x 2 table is empty"""
    t = np.asarray(table, dtype=np.float64).reshape(5, 5)
    r = _top2(t.sum(axis=1)); c = _top2(t.sum(axis=0))
    a, b, cc, d = t[r[0], c[0]], t[r[0], c[1]], t[r[1], c[0]], t[r[1], c[1]]
    den = (a + b) * (cc + d) * (a + cc) * (b + d)
    return 0.0 if den <= 0 else float((a * d - b * cc) / np.sqrt(den))


def linked_sites(tables, min_phi=DEFAULTS["min_phi"], single_min_frac=DEFAULTS["single_min_frac"], site_counts=None):
    """-> bool [S]: the sites that are kept.  tables [S, S, 5, 5] as Api.phase_pair_tables returns them.  A site is kept when |phi| >= min_phi with at least one other
    site.  A site without such a partner is kept only if its two most frequent alleles are both bases (no del) and the minor one holds at least single_min_frac of the two.
    site_counts [S, 5]: the allele counts of every site over all its reads (split() takes them from the genotypes); without them they are the marginals of the site's table
    with its neighbour."""
    t = np.asarray(tables); S = t.shape[0] if t.ndim == 4 else int(round((t.size // 25) ** 0.5))
    t = t.reshape(S, S, 5, 5)
    keep = np.zeros(S, dtype=bool)
    for s in range(S):
        for u in range(s + 1, S):
            if abs(pair_phi(t[s, u])) >= min_phi - _EPS:
                keep[s] = keep[u] = True
    if site_counts is None:
        site_counts = np.zeros((S, 5), dtype=np.int64)
        for s in range(S):
            if s + 1 < S: site_counts[s] = t[s, s + 1].sum(axis=1)
            elif S > 1: site_counts[s] = t[s - 1, s].sum(axis=0)
    sc = np.asarray(site_counts, dtype=np.int64).reshape(S, 5)
    for s in np.nonzero(~keep)[0]:
        a, b = _top2(sc[s]); n = int(sc[s, a] + sc[s, b])
        keep[s] = a < GENO_DEL and b < GENO_DEL and sc[s, b] > 0 and sc[s, b] >= single_min_frac * n - _EPS
    return keep


def haplotypes(geno, kept, min_hap_reads=DEFAULTS["min_hap_reads"], min_hap_frac=DEFAULTS["min_hap_frac"], max_haps=DEFAULTS["max_haps"], allowed=None):
    """geno [R, S] codes, kept = indices (or a bool mask) of the kept sites -> (alleles [H, K] uint8, counts [H]) or None.  Among the reads whose codes at ALL kept sites are
    <= GENO_DEL, every distinct allele string seen at least max(min_hap_reads, ceil(min_hap_frac * such reads)) times is a haplotype; order: count descending, then the string;
    at most max_haps; fewer than two: None (no split).  allowed [K, 2] (optional): only strings that carry one of these two alleles at every kept site are candidates - the
    linkage test has looked at a site's two most frequent alleles only (the bound still counts every fully covered read)."""
    g = np.asarray(geno, dtype=np.uint8); kept = np.asarray(kept)
    if kept.dtype == bool: kept = np.nonzero(kept)[0]
    if len(kept) == 0 or g.shape[0] == 0: return None
    sub = g[:, kept]; full = sub[(sub <= GENO_DEL).all(axis=1)]
    if len(full) == 0: return None
    n_full = len(full)
    if allowed is not None:
        al = np.asarray(allowed, dtype=np.uint8).reshape(len(kept), 2)
        full = full[((full == al[:, 0]) | (full == al[:, 1])).all(axis=1)]
        if len(full) == 0: return None
    strings, cnt = np.unique(full, axis=0, return_counts=True)            # rows come out in lexicographic order
    ok = cnt >= max(float(min_hap_reads), min_hap_frac * n_full - _EPS)
    strings, cnt = strings[ok], cnt[ok]
    o = np.argsort(-cnt, kind="stable")[:min(int(max_haps), PHASE_MAX_HAPS)]
    if len(o) < 2: return None
    return strings[o].astype(np.uint8), cnt[o].astype(np.int64)


def apply_margin(best, dist, dist2, min_margin=DEFAULTS["min_margin"]):
    """the haplotype of every read, -1 where it joins none: best == -1, or the second-nearest haplotype is fewer than min_margin sites further away than the nearest"""
    best = np.asarray(best, dtype=np.int8); out = best.copy()
    out[(best < 0) | (np.asarray(dist2, dtype=np.int64) - np.asarray(dist, dtype=np.int64) < min_margin)] = -1
    return out


def split_many(api, rs, centres, lists, supports=None, k=13, w=20, clip=False, **policy):
    """The haplotypes of several centres with ONE call each of phase_genotypes, phase_pair_tables and phase_assign.  centres: the final sequences; lists: the pooled reads
    of each (the polisher's lists); supports: their [len, 8] counters (computed here when None).  -> (one entry per centre: None, or dict(sites [K] centre positions,
    alleles [H, K], n_reads [H], assign [len(list)] int8 with -1 = in no haplotype), strand [per listed read] int8)."""
    unknown = set(policy) - set(DEFAULTS)
    if unknown: raise TypeError("phase.split_many: unknown policy argument(s) %s" % sorted(unknown))
    P = dict(DEFAULTS, **policy)
    n = len(centres)
    grp_off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
    ro = (np.concatenate(lists) if n else np.zeros(0)).astype(np.uint32)
    cen = ReadSet.from_strings(list(centres))
    if supports is None:
        counts, cen_off, _, _ = api.consensus_support(cen, rs, grp_off, read_order=ro, k=k, w=w, clip=clip)
        supports = [counts[int(cen_off[i]):int(cen_off[i + 1])] for i in range(n)]
    sites = [candidate_sites(supports[i], centres[i], P["min_alt_frac"], P["min_alt_reads"]) for i in range(n)]
    site_off = np.concatenate(([0], np.cumsum([len(s) for s in sites]))).astype(np.uint64)
    site_pos = (np.concatenate(sites) if n else np.zeros(0)).astype(np.uint32)
    geno, geno_off, strand = api.phase_genotypes(cen, rs, grp_off, site_off, site_pos, read_order=ro, k=k, w=w, clip=clip)
    tables, tab_off = api.phase_pair_tables(geno, grp_off, site_off)
    haps = [None] * n; hap_rows = []; hap_off = np.zeros(n + 1, dtype=np.uint64)
    for i in range(n):
        S = len(sites[i]); R = len(lists[i])
        if S and R:
            g = geno[int(geno_off[i]):int(geno_off[i + 1])].reshape(R, S)
            sc = np.stack([np.bincount(g[:, s], minlength=8)[:5] for s in range(S)])
            keep = linked_sites(tables[int(tab_off[i]):int(tab_off[i + 1])].reshape(S, S, 5, 5), P["min_phi"], P["single_min_frac"], site_counts=sc)
            allowed = [_top2(sc[s]) for s in np.nonzero(keep)[0]] if P["top2_only"] else None
            hp = haplotypes(g, keep, P["min_hap_reads"], P["min_hap_frac"], P["max_haps"], allowed=allowed)
            if hp is not None:
                kept = np.nonzero(keep)[0]
                full = np.full((len(hp[0]), S), HAP_ANY, dtype=np.uint8); full[:, kept] = hp[0]
                haps[i] = (kept, hp[0]); hap_rows.append(full.ravel())
        hap_off[i + 1] = hap_off[i] + (0 if haps[i] is None else len(haps[i][1]))
    out = [None] * n
    if hap_rows:
        best, dist, dist2 = api.phase_assign(geno, grp_off, site_off, hap_off, np.concatenate(hap_rows))
        for i in range(n):
            if haps[i] is None: continue
            a, b = int(grp_off[i]), int(grp_off[i + 1]); kept, alleles = haps[i]
            assign = apply_margin(best[a:b], dist[a:b], dist2[a:b], P["min_margin"])
            n_reads = np.bincount(assign[assign >= 0], minlength=len(alleles)).astype(np.int64)
            if (n_reads == 0).any(): continue                             # (a margin above 1 can empty a haplotype: no split then)
            out[i] = dict(sites=sites[i][kept].astype(np.uint32), alleles=alleles, n_reads=n_reads, assign=assign)
    return out, strand


def split(api, rs, centre, reads, support=None, k=13, w=20, clip=False, **policy):
    """split_many for one centre and its pooled reads -> None or dict(sites, alleles, n_reads, assign)"""
    return split_many(api, rs, [centre], [np.asarray(reads)], None if support is None else [support], k=k, w=w, clip=clip, **policy)[0][0]


def build(api, rs, centres, lists, poa_prm, polish_prm, supports=None, k=13, w=20, clip=False, host_rs=None, **policy):
    """split_many + the sequences of the haplotypes: ONE poa_consensus call and (polish_prm not None) ONE polish call over the haplotype read groups of all centres that
    split, with the parameters of the clusters' own draft and polish; the backbone of a haplotype is its draft.  The reads of a pooled list come in both strands (the
    clusters of the two strands were merged), so the two calls see a host copy of the haplotypes' reads only, oriented by the strand the genotype call reports (host_rs: the
    host copy of a device-resident rs that does not carry one).  The entries gain draft [H], polished [H] and used [H] (reads the polisher used; without polishing the
    reads of the haplotype)."""
    from . import strand as strand_mod
    from .hostutil import subset_reads
    out, st = split_many(api, rs, centres, lists, supports, k=k, w=w, clip=clip, **policy)
    groups = []; flips = []
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists])))
    for i, e in enumerate(out):
        if e is None: continue
        l = np.asarray(lists[i]); s = st[int(off[i]):int(off[i + 1])]
        for h in range(len(e["alleles"])):
            m = e["assign"] == h
            groups.append(l[m]); flips.append(s[m] == 1)
    if not groups: return out
    host = rs if rs.mem == MEM_HOST else (host_rs if host_rs is not None else (rs.keep if isinstance(rs.keep, dict) else {}).get("host"))
    if host is None and isinstance(rs.keep, dict) and rs.keep.get("seq") is not None:          # torch-backed device read set: download it
        t = rs.keep
        host = ReadSet(t["seq"].cpu().numpy(), None if t.get("qual") is None else t["qual"].cpu().numpy(), t["off"].cpu().numpy().astype(np.uint64))
    if host is None or host.mem != MEM_HOST: raise ValueError("phase.build needs a host copy of the reads (host_rs) beside a device-resident read set")
    g_off = np.concatenate(([0], np.cumsum([len(x) for x in groups]))).astype(np.uint64)
    oriented = strand_mod.orient_reads(subset_reads(host, np.concatenate(groups)), np.concatenate(flips))
    ro = np.arange(oriented.n, dtype=np.uint32)
    drafts = api.poa_consensus(oriented, g_off, poa_prm, read_order=ro)
    polished = list(drafts); used = [len(x) for x in groups]
    if polish_prm is not None:
        polished, used = api.polish(ReadSet.from_strings(list(drafts)), oriented, g_off, polish_prm, read_order=ro)
    x = 0
    for e in out:
        if e is None: continue
        H = len(e["alleles"])
        e["draft"] = list(drafts[x:x + H]); e["polished"] = list(polished[x:x + H]); e["used"] = [int(u) for u in used[x:x + H]]; x += H
    return out


def allele_string(row):
    return "".join(ALLELES[int(c)] for c in row)


def table_rows(cluster_ids, entries):
    """the rows of haplotypes.tsv: cluster id, haplotype index, reads, site positions (1-based, comma-separated), alleles over ACGT-"""
    rows = []
    for cid, e in zip(cluster_ids, entries):
        if e is None: continue
        pos = ",".join(str(int(p) + 1) for p in e["sites"])
        for h in range(len(e["alleles"])):
            rows.append((str(cid), str(h), str(int(e["n_reads"][h])), pos, allele_string(e["alleles"][h])))
    return rows


def write_table(path, rows):
    with open(path, "w") as f:
        f.write("cluster_id\thaplotype\treads\tsites\talleles\n")
        for r in rows: f.write("\t".join(r) + "\n")


def policy_from_args(args):
    """the --hap_* flags as policy arguments of split_many"""
    return dict(min_alt_frac=args.hap_min_alt_frac, min_hap_reads=args.hap_min_reads, min_phi=args.hap_min_phi, max_haps=args.hap_max)


def check_args(args):
    """the range checks of the --hap_* flags -> an error text or None"""
    if not 0.0 < args.hap_min_alt_frac <= 0.5: return "--hap_min_alt_frac is a fraction in (0, 0.5]."
    if args.hap_min_reads < 1: return "--hap_min_reads must be at least 1."
    if not 0.0 <= args.hap_min_phi <= 1.0: return "--hap_min_phi is a coefficient in [0, 1]."
    if not 2 <= args.hap_max <= PHASE_MAX_HAPS: return "--hap_max must be 2..%d." % PHASE_MAX_HAPS
    return None
