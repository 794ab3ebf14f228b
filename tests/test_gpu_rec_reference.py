"""GPU: the five consumers of the store pass (ngsid_rec_walk: strand call, oriented copies, the REC instances of k_ed_align) - consensus_support, read_cigars (with and
without merge_m), phase_genotypes, hp_runs, error_profile - against their references with the columns and strands of tests/columns_reference.py, on the edge families
of tests/rec_cases.py.  No oracle is involved; every comparison is exact (integers).  include/ngsid.h: results never depend on the scheduling options.

One (family, setting) per test.  Which instance or launch a setting aims at (read from ed_align_route in csrc/k_ed_align.hip; B = register-resident blocks of 64 rows,
WIN = the sliding-window instances, all with REC):
  default   pack, ends, ties: B4.  clip (clip = 1): the one CLIP instance (B16, unbanded); its contrast call: B4.  inst: 256 -> B4; 257, 512 -> B8; 513, 768 -> B12;
            769 ... 1024 -> B16 banded; 1025, 2752 -> WIN B8 (band 64 + n / 32 <= 150); 2784 -> WIN B16 (band 151 -> 64 + n / 16).  band: B4 / B8 / B16 with the
            default band 64 + n / 32: the pairs of K = 150 beyond it go to the unbanded launch by pair list.  class (4 096 pairs or more, longest read > 256): the class
            launches B4, B8, WIN B6 for 513 - 896 (two index lists in one launch), B16 above 896, then the retry launch WIN B8 with band 180 and the unbanded B16.
  band0     no band, no fallback: inst -> B4 / B8 / B12 / B16 with all blocks resident (2752, 2784: 44 blocks in groups of 16); class: B12 and B16 class launches.
  band12    nearly every pair with an edit run leaves the band: inst, band -> the unbanded launch by pair list does the work; (class: band40 does that).
  band40    band: K = 12 inside, K = 40 at the edge, K = 150 outside.  class: WIN B6 with a narrow band, most pairs to the retry launch, the blocks beyond 180 unbanded.
  band150   inst 1025 ... 2784 -> WIN B8 with a set band; band: K = 150 at the edge; class: 100 < band <= 150 -> WIN B8 instead of WIN B6 for 513 - 896.
  band400   inst 1025 ... 2784 -> WIN B16 (a set band above 150, capped at 400); class: band > 150 -> no window instance below 897: B12 and B16, fallback without retry.
  win_all0  class: B12 for 513 - 768 and B16 for 769 - 896 instead of the window instance.        win6_0  class: WIN B8 instead of WIN B6.
  noclass   class: ONE launch (B16) over bundles that mix the length classes in pair order, then the unbanded launch.
  budget1   class with support_budget_mb = 1: chunks of 1 927 rows (385 with read positions) - chunk boundaries inside groups and inside bundles; fewer than 4 096 pairs
            a chunk, so B16 banded + the unbanded launch, whose rows of the path matrix are written by a later launch of the same chunk.
A mismatch names the case, the listed read, its tag, (n, m), the strand, and the lane and bundle of its pair in pair order.
"""
import numpy as np
import pytest
import rec_cases
import rec_expected as rx

pytestmark = pytest.mark.gpu

SETTINGS = {"default": {}, "win_all0": {"ed_win_all": 0}, "win6_0": {"ed_win6": 0}, "noclass": {"align_noclass": 1}, "budget1": {}}
for _b in (0, 12, 40, 150, 400): SETTINGS["band%d" % _b] = {"ed_band": _b}
MATRIX = {"pack": ["default"], "ends": ["default"], "ties": ["default"], "clip": ["default"],
          "inst": ["default", "band0", "band12", "band150", "band400"],
          "band": ["default", "band0", "band12", "band40", "band150", "band400"],
          "class": ["default", "band0", "band40", "band150", "band400", "win_all0", "win6_0", "noclass", "budget1"]}


def where(case, x, strand):
    """the words of a mismatch for listed read x"""
    g = rx.group_of(case, x)
    rank = int((np.asarray(strand[:x]) >= 0).sum())
    return "listed read %d of group %d, tag %s, n %d, m %d, strand %d, lane %d of bundle %d in pair order" % (
        x, g, case.tags[x], len(case.reads[int(case.read_order[x])]), len(case.centres[g]), strand[x], rank % 64, rank // 64)


def first_read(case, strand, rows):
    """rows: a bool per listed read -> words for the first True"""
    bad = np.nonzero(rows)[0]
    return "%d listed reads differ; first: %s" % (len(bad), where(case, int(bad[0]), strand))


def check_strand(case, what, got, exp, note):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (case.name, what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        x = int(np.nonzero(got != exp)[0][0])
        pytest.fail("%s%s: %s: strand: %s; got %d" % (case.name, note, what, first_read(case, exp, got != exp), got[x]))


def check_cigars(case, what, got, exp, note):
    aln, op_off, ops, strand = got; e_aln, e_off, e_ops, e_strand = exp
    check_strand(case, what, strand, e_strand, note)
    assert aln.dtype == np.int32 and op_off.dtype == np.uint64 and ops.dtype == np.uint32 and aln.shape == e_aln.shape and op_off.shape == e_off.shape
    rows = (aln != e_aln).any(axis=1) | (np.diff(op_off.astype(np.int64)) != np.diff(e_off.astype(np.int64)))
    for x in np.nonzero(~rows)[0]:
        if not np.array_equal(ops[int(op_off[x]):int(op_off[x + 1])], e_ops[int(e_off[x]):int(e_off[x + 1])]): rows[x] = True
    if rows.any():
        x = int(np.nonzero(rows)[0][0])
        txt = lambda o: "".join("%d%s" % (v >> 4, "MIDNSHP=X"[v & 15]) for v in o.tolist())
        pytest.fail("%s%s: %s: %s\n  aln got %s expected %s\n  ops got      %s\n  ops expected %s" % (case.name, note, what, first_read(case, e_strand, rows), aln[x].tolist(), e_aln[x].tolist(),
                    txt(ops[int(op_off[x]):int(op_off[x + 1])])[:400], txt(e_ops[int(e_off[x]):int(e_off[x + 1])])[:400]))
    assert np.array_equal(op_off, e_off) and np.array_equal(ops, e_ops), (case.name, what)


def check_geno(case, got, exp, note):
    geno, geno_off, strand = got; e_geno, e_off, e_strand = exp
    check_strand(case, "phase_genotypes", strand, e_strand, note)
    assert geno.dtype == np.uint8 and np.array_equal(geno_off, e_off) and geno.shape == e_geno.shape
    if np.array_equal(geno, e_geno): return
    for g in range(len(case.centres)):
        a, b = int(case.grp_off[g]), int(case.grp_off[g + 1]); S = int(case.site_off[g + 1] - case.site_off[g])
        if a == b or S == 0: continue
        u = geno[int(e_off[g]):int(e_off[g + 1])].reshape(b - a, S); v = e_geno[int(e_off[g]):int(e_off[g + 1])].reshape(b - a, S)
        if not np.array_equal(u, v):
            rows = np.zeros(len(e_strand), dtype=bool); rows[a:b] = (u != v).any(axis=1)
            x = int(np.nonzero(rows)[0][0]); s = np.nonzero(u[x - a] != v[x - a])[0]
            sites = case.site_pos[int(case.site_off[g]):int(case.site_off[g + 1])]
            pytest.fail("%s%s: phase_genotypes: %s\n  sites %s got %s expected %s" % (case.name, note, first_read(case, e_strand, rows), sites[s].tolist()[:10], u[x - a][s].tolist()[:10], v[x - a][s].tolist()[:10]))


def check_table(case, what, names, got, exp, per_group, strand, note):
    """outputs summed over reads: names the group and the first entries that differ, and the group's first read with a strand (every read of a group of copies is that read)"""
    for nm, u, v in zip(names, got, exp):
        if v is None: assert u is None; continue
        assert u.dtype == v.dtype and u.shape == v.shape, (case.name, what, nm, u.dtype, v.dtype, u.shape, v.shape)
        if np.array_equal(u, v): continue
        flat = np.nonzero((u != v).reshape(len(u), -1).any(axis=1))[0]; r = int(flat[0])
        g = per_group(r)
        reads = [x for x in range(int(case.grp_off[g]), int(case.grp_off[g + 1])) if strand[x] >= 0]
        pytest.fail("%s%s: %s: %s differs in %d rows; first: row %d (group %d, %d listed reads, centre of %d letters); the group's first read with a strand: %s\n  got      %s\n  expected %s"
                    % (case.name, note, what, nm, len(flat), r, g, int(case.grp_off[g + 1] - case.grp_off[g]), len(case.centres[g]), where(case, reads[0], strand) if reads else "none",
                       u[r].tolist(), v[r].tolist()))


def run_case(api, case, note):
    cen, rs = rx.read_sets(case)
    kw = dict(read_order=case.read_order, k=case.k, w=case.w, clip=case.clip)
    # the per-read outputs first: they name the read
    check_cigars(case, "read_cigars", api.read_cigars(cen, rs, case.grp_off, **kw), rx.expected(case, "cigar"), note)
    check_cigars(case, "read_cigars merge_m", api.read_cigars(cen, rs, case.grp_off, merge_m=True, **kw), rx.expected(case, "cigar_m"), note)
    check_geno(case, api.phase_genotypes(cen, rs, case.grp_off, case.site_off, case.site_pos, **kw), rx.expected(case, "geno"), note)
    strand = rx.expected(case, "cigar")[3]
    counts, cen_off, used, st = api.consensus_support(cen, rs, case.grp_off, **kw)
    e_counts, e_off, e_used, e_st = rx.expected(case, "support")
    check_strand(case, "consensus_support", st, e_st, note)
    assert np.array_equal(cen_off, e_off)
    check_table(case, "consensus_support", ("n_used",), (used,), (e_used,), lambda r: r, strand, note)
    check_table(case, "consensus_support", ("counts",), (counts,), (e_counts,), lambda r: int(np.searchsorted(e_off, r, side="right")) - 1, strand, note)
    hist, st = api.hp_runs(cen, rs, case.grp_off, case.run_off, case.run_start, **kw)
    e_hist, e_st = rx.expected(case, "hp")
    check_strand(case, "hp_runs", st, e_st, note)
    check_table(case, "hp_runs", ("hist",), (hist,), (e_hist,), lambda r: int(np.searchsorted(case.run_off, r, side="right")) - 1, strand, note)
    cnt, qtab, st = api.error_profile(cen, rs, case.grp_off, **kw)
    e_cnt, e_qtab, e_st = rx.expected(case, "errprof")
    check_strand(case, "error_profile", st, e_st, note)
    check_table(case, "error_profile", ("counts", "qtab"), (cnt, qtab), (e_cnt, e_qtab), lambda r: r, strand, note)


class own_context:
    """a context of the test's own.  Its traceback scratch is bounded at 2 GB (the class launches reserve theirs by the budget, by default a quarter of the free device
    memory, not by the call: 64 bundles need 1.1 GB), and before it is closed its scratch and the process's cache of freed blocks go back to the driver: the tests that
    follow in this process start child processes on the same device."""
    def __init__(self, options):
        from ngspeciesid_amd import runtime
        self.api = runtime.new_api(options=dict(options, scratch_budget_mb=2048))

    def __enter__(self):
        return self.api

    def __exit__(self, *exc):
        try: self.api.set_option("release_scratch", 1)
        finally: self.api.close()


@pytest.mark.parametrize("family,setting", [(f, s) for f in sorted(MATRIX) for s in MATRIX[f]])
def test_family_equals_reference(gpu_api, family, setting):
    with own_context(SETTINGS[setting]) as api:
        if setting == "budget1": api.set_option("support_budget_mb", 1)
        for case in rec_cases.cases(family):
            run_case(api, case, " [%s]" % setting)


def test_pack_again_after_a_longer_centre(gpu_api):
    """the path matrix, the read positions and the traceback scratch only grow, and the row stride follows the longest centre of the CALL: a call with a 2 800-letter
    centre (stride 352 dwords), then the row-packing family (stride 72) on the same context"""
    long_case = rec_cases.cases("inst")[-1]
    (pack,) = rec_cases.cases("pack")
    assert max(len(c) for c in long_case.centres) >= 2800 > 5 * max(len(c) for c in pack.centres)
    with own_context({}) as api:
        run_case(api, pack, " [fresh context]")
        run_case(api, long_case, " [2 800-letter centre]")
        run_case(api, pack, " [after the longer centre]")
