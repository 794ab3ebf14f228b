"""The definition of the three calls of include/ngsid_phase.h restated from the CPU oracle's parts.  Test infrastructure - never imported by the product.

Genotypes: the strands and the counted columns are those of tests/support_reference.py (strands of ongsid_polish_trace_aln, columns of ongsid_i_ed_ops, count_read's clip
rules) - one read's counters ARE its genotype: at a base it counts, exactly one of agree / sub_* / del is 1, or none of them (a mismatch with a read base outside ACGT).
Pair tables and assignment: numpy, here.  PhaseAdapter gives an oracle-backed Api the three phase_* methods (and consensus_support), so the pipeline runs on the CPU."""
import numpy as np
from ngspeciesid_amd._capi import ReadSet, phase_offsets
from support_reference import support_reference, strands, strand_list, count_read, _COMP

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i; _CODE[_c + 32] = _i


def read_genotype(oracle, read, centre, sites, clip, source=None):
    """codes of ONE oriented read at the centre positions `sites`"""
    cnt = np.zeros((len(centre), 8), dtype=np.uint32)
    out = np.full(len(sites), 7, dtype=np.uint8)
    if len(sites) == 0 or not count_read(oracle, cnt, read, centre, clip, source): return out
    c = cnt[np.asarray(sites, dtype=np.int64)]
    assert c[:, :7].max() <= 1
    for j in range(len(sites)):
        if c[j, 0] == 0: continue
        if c[j, 1]: out[j] = _CODE[centre[int(sites[j])]]
        elif c[j, 2:6].any(): out[j] = int(np.argmax(c[j, 2:6]))
        elif c[j, 6]: out[j] = 4
        else: out[j] = 5
    return out


def genotypes_reference(oracle, centres, rs, grp_off, site_off, site_pos, read_order=None, k=13, w=20, clip=False, source=None):
    """-> (geno, geno_off, strand) as Api.phase_genotypes returns them; source as in support_reference"""
    grp_off = np.asarray(grp_off, dtype=np.uint64); site_off = np.asarray(site_off, dtype=np.uint64); site_pos = np.asarray(site_pos, dtype=np.uint32)
    ng = len(grp_off) - 1; nl = int(grp_off[-1])
    ro = np.arange(nl, dtype=np.uint32) if read_order is None else np.ascontiguousarray(read_order, dtype=np.uint32)
    geno_off, _ = phase_offsets(grp_off, site_off)
    geno = np.full(int(geno_off[-1]), 7, dtype=np.uint8); strand = np.full(nl, -1, dtype=np.int8)
    for g in range(ng):
        a, b = int(grp_off[g]), int(grp_off[g + 1])
        if a == b: continue
        sites = site_pos[int(site_off[g]):int(site_off[g + 1])]
        st = strand_list(oracle, source, [centres[g]], rs, np.array([0, b - a], dtype=np.uint64), ro[a:b].copy(), k, w)
        strand[a:b] = st
        centre = np.frombuffer(centres[g].encode(), dtype=np.uint8)
        block = geno[int(geno_off[g]):int(geno_off[g + 1])].reshape(b - a, len(sites))
        for x, r in enumerate(ro[a:b].tolist()):
            if st[x] < 0 or len(sites) == 0: continue
            read = rs.seq[int(rs.off[r]):int(rs.off[r + 1])]
            if st[x] == 1: read = _COMP[read[::-1]]
            block[x] = read_genotype(oracle, np.ascontiguousarray(read), centre, sites, clip, source)
    return geno, geno_off, strand


def pair_tables_numpy(geno, grp_off, site_off):
    """-> (tables, tab_off) as Api.phase_pair_tables returns them"""
    grp_off = np.asarray(grp_off, dtype=np.uint64); site_off = np.asarray(site_off, dtype=np.uint64)
    geno_off, tab_off = phase_offsets(grp_off, site_off)
    tables = np.zeros(int(tab_off[-1]), dtype=np.uint32)
    for g in range(len(grp_off) - 1):
        R = int(grp_off[g + 1] - grp_off[g]); S = int(site_off[g + 1] - site_off[g])
        if S < 2: continue
        m = np.asarray(geno)[int(geno_off[g]):int(geno_off[g + 1])].reshape(R, S).astype(np.int64)
        t = tables[int(tab_off[g]):int(tab_off[g + 1])].reshape(S, S, 25)
        for s in range(S):
            for u in range(s + 1, S):
                ok = (m[:, s] <= 4) & (m[:, u] <= 4)
                t[s, u] = np.bincount(m[ok, s] * 5 + m[ok, u], minlength=25)
    return tables, tab_off


def assign_numpy(geno, grp_off, site_off, hap_off, hap_alleles):
    """-> (best, dist, dist2) as Api.phase_assign returns them"""
    grp_off = np.asarray(grp_off, dtype=np.uint64); site_off = np.asarray(site_off, dtype=np.uint64); hap_off = np.asarray(hap_off, dtype=np.uint64)
    geno_off, _ = phase_offsets(grp_off, site_off); hal = np.asarray(hap_alleles, dtype=np.uint8).ravel()
    nl = int(grp_off[-1]); best = np.full(nl, -1, dtype=np.int8); dist = np.full(nl, 255, dtype=np.uint8); dist2 = np.full(nl, 255, dtype=np.uint8)
    hp = 0
    for g in range(len(grp_off) - 1):
        a = int(grp_off[g]); R = int(grp_off[g + 1]) - a; S = int(site_off[g + 1] - site_off[g]); H = int(hap_off[g + 1] - hap_off[g])
        al = hal[hp:hp + H * S].reshape(H, S); hp += H * S
        if not (R and S and H): continue
        m = np.asarray(geno)[int(geno_off[g]):int(geno_off[g + 1])].reshape(R, S)
        for x in range(R):
            cov = m[x] <= 4
            if not cov.any(): continue
            d = [int((cov & (al[h] != 255) & (al[h] != m[x])).sum()) for h in range(H)]
            b = min(range(H), key=lambda h: (d[h], h))
            best[a + x] = b; dist[a + x] = d[b]; dist2[a + x] = min([d[h] for h in range(H) if h != b], default=255)
    return best, dist, dist2


class PhaseAdapter:
    """an oracle-backed Api with consensus_support and the three phase_* methods answered by the reference definitions; everything else is the oracle's"""
    def __init__(self, oracle):
        self._o = oracle

    def __getattr__(self, name):
        return getattr(self._o, name)

    @staticmethod
    def _centres(centres):
        return [centres.get(i)[0] for i in range(centres.n)]

    def consensus_support(self, centres, rs, grp_off, read_order=None, k=13, w=20, clip=False):
        return support_reference(self._o, self._centres(centres), rs, grp_off, read_order, k, w, clip)

    def phase_genotypes(self, centres, rs, grp_off, site_off, site_pos, read_order=None, k=13, w=20, clip=False):
        return genotypes_reference(self._o, self._centres(centres), rs, grp_off, site_off, site_pos, read_order, k, w, clip)

    def phase_pair_tables(self, geno, grp_off, site_off):
        return pair_tables_numpy(geno, grp_off, site_off)

    def phase_assign(self, geno, grp_off, site_off, hap_off, hap_alleles):
        return assign_numpy(geno, grp_off, site_off, hap_off, hap_alleles)
