"""The adversarial clustering cases (tests/cluster_cases.py) on the CPU: the oracle's sequential loop gives what the reference's own reads_to_clusters gave
(tests/golden/cluster_edges.npz, oracle/make_golden_cluster_edges.py) - membership, status, the mapping-stage triple of every read, the counters, the p-table error - and every
case still reaches the mechanism it was built for (conditions on fixture and oracle data only, so that a case cannot silently degrade)."""
import ctypes as C
import math
import numpy as np
import pytest
import cluster_cases as CC
from ngspeciesid_amd._capi import NgsidError

ST_NEWREP, ST_MAPPED, ST_ALIGNED, ST_SHORT, ST_SEEDED = 0, 1, 2, 3, 4
ERR_NO_PTABLE = -7
FROZEN = {f.name: f for f in CC.load_frozen()}


def run_oracle(oracle, fz, c, trace=True):
    """-> (rep_of, hpc_err, status, counters, (best, nshared, ratio)) or the NgsidError code"""
    prm, kw = fz.call(c)
    n = fz.rs.n
    bm = np.full(n, -2, dtype=np.int32); ns = np.zeros(n, dtype=np.int32); ra = np.zeros(n)
    if trace: oracle.lib.ongsid_debug_enable_trace(bm.ctypes.data_as(C.c_void_p), ns.ctypes.data_as(C.c_void_p), ra.ctypes.data_as(C.c_void_p), C.c_uint64(n))
    try:
        rep, herr, st, cnt = oracle.cluster_greedy(fz.rs, prm, **kw)
    except NgsidError as e:
        return e.code
    finally:
        oracle.lib.ongsid_debug_enable_trace(None, None, None, C.c_uint64(0))
    return rep, herr, st, cnt, (bm, ns, ra)


@pytest.mark.parametrize("name", sorted(FROZEN))
def test_oracle_equals_the_reference(oracle, name):
    fz = FROZEN[name]; f = fz.f
    for c, tag in enumerate(fz.tags):
        got = run_oracle(oracle, fz, c)
        if f["error"][c]:
            assert got == ERR_NO_PTABLE, (tag, "the reference raised KeyError")
            continue
        assert not isinstance(got, int), (tag, got)
        rep, herr, st, cnt, (bm, ns, ra) = got
        assert np.array_equal(rep, f["rep_of"][c]), tag
        assert np.array_equal(st, f["status"][c]), tag
        assert [int(x) for x in cnt[:3]] == [int(x) for x in f["counters"][c]], tag
        items = (st != ST_SEEDED) & (st != ST_SHORT)            # reads that reached get_best_cluster (cluster.py:302)
        assert np.array_equal(bm[items], f["tr_best"][c][items]) and np.array_equal(ns[items], f["tr_ns"][c][items]), tag
        assert np.array_equal(ra[items], f["tr_ratio"][c][items]), tag
        assert int(cnt[3]) == int((st == ST_NEWREP).sum())
        if f["has_known"][c]:
            k = ~np.isnan(f["known"][c]); assert np.array_equal(herr[k & (st != ST_SHORT)], f["known"][c][k & (st != ST_SHORT)]), tag


def test_generators_reproduce_the_fixture(oracle):
    cases = CC.all_cases(oracle)
    assert sorted(c.name for c in cases) == sorted(FROZEN)
    for case in cases:
        fz = FROZEN[case.name]
        assert [fz.rs.get(i) for i in range(fz.rs.n)] == list(zip(case.seqs, case.quals)), case.name
        assert fz.acc == case.acc and (fz.k, fz.w) == (case.k, case.w)
        if case.name == "threshold_equalities":
            assert fz.tags == [c.tag for c in case.calls] + list(CC.THRESHOLD_CALLS)
            continue
        assert fz.tags == [c.tag for c in case.calls]
        for c, call in enumerate(case.calls):
            assert [float(call.prm[key]) for key in CC.PRM_KEYS] == fz.f["prm"][c].tolist()
            assert (call.prev_batch is None) == (not fz.f["has_prev"][c]) and (call.prev_batch is None or np.array_equal(call.prev_batch, fz.f["prev"][c]))
            assert (call.known_err is None) == (not fz.f["has_known"][c]) and (call.known_err is None or np.array_equal(call.known_err, fz.f["known"][c], equal_nan=True))


# ------------------------------------------------------------------------------------------------ each case reaches its mechanism
def test_round2_every_boundary_on_both_axes(oracle):
    """(a) for the read and for the representative: an error rate on each side of each of the 14 row changes of round(e, 2) and inside both clamps - the expected rows come from
    CPython's round(), never from the table header - and the pair maps in every call (the cell with p = 0 was read).  The table tells cells apart: the value of a neighbouring
    cell gives another status, the transposed cell the p-table error."""
    fz = FROZEN["round2_boundaries"]; f = fz.f
    assert not f["error"].any() and (f["status"][:, 1] == ST_MAPPED).all()
    for axis, col in (("read", 1), ("rep", 0)):
        sel = [c for c, t in enumerate(fz.tags) if t.startswith(axis)]
        e = f["known"][sel, col]
        rows = [CC.round2_index(float(x)) for x in e]
        assert set(rows) == set(range(1, 16))
        srt = np.sort(e)
        for b in range(1, 15):                                   # boundary between rows b and b + 1: two neighbouring doubles on its two sides
            lo = max(x for x in srt if CC.round2_index(float(x)) == b); hi = min(x for x in srt if CC.round2_index(float(x)) == b + 1)
            assert math.nextafter(lo, 1.0) == hi, (axis, b)
        assert min(e) == 0.0 and max(e) == 1.0 and any(0.15 < x < 0.16 and round(x, 2) == 0.16 for x in e) and any(0.004 < x < 0.005 for x in e)
    from ngspeciesid_amd._capi import cluster_params
    for c in (5, 20, 60, 90):
        prm, kw = fz.call(c)
        i, j = CC.round2_index(float(kw["known_err"][1])), CC.round2_index(float(kw["known_err"][0]))
        assert i != j
        t = CC.round2_table(kw["known_err"][1], kw["known_err"][0]).reshape(15, 15)
        shifted = t.copy(); shifted[i - 1, j - 1] = 1.0          # what a neighbouring cell holds
        st = oracle.cluster_greedy(fz.rs, cluster_params(k=13, w=20, p_shared=shifted.reshape(225)), **kw)[2]
        assert st[1] != ST_MAPPED
        with pytest.raises(NgsidError) as ei:                     # a transposed lookup meets NaN
            oracle.cluster_greedy(fz.rs, cluster_params(k=13, w=20, p_shared=t.T.copy().reshape(225)), **kw)
        assert ei.value.code == ERR_NO_PTABLE


def test_tied_candidates_wrap_the_cache():
    """(b) a read asked for more than NCACHE = 4 aligner pairs and still founded a cluster, behind a founder it shares >= min_shared minimizers with"""
    fz = FROZEN["tied_candidates_beyond_cache"]; f = fz.f
    q = fz.rs.n - 1
    assert f["pairs"][0][q] > 4 and f["status"][0][q] == ST_NEWREP
    assert f["status"][0][q - 1] == ST_NEWREP and f["pairs"][0][q - 1] == 0 and f["tr_ns"][0][q] >= 5
    assert f["pairs"][0][5] > 4                                   # the sixth representative walked the five before it


def test_accession_order_beats_slot_order():
    """(c) both queries went to the LATER of the two tied representatives, one by the mapping and one by the alignment criterion"""
    fz = FROZEN["accession_tiebreak"]; f = fz.f
    assert f["status"][0].tolist() == [ST_NEWREP, ST_NEWREP, ST_MAPPED, ST_ALIGNED]
    assert f["rep_of"][0].tolist() == [0, 1, 1, 1] and fz.acc_rank[1] > fz.acc_rank[0]


def test_threshold_equalities_flip_the_status():
    """(d) at the ratio itself the strict mapping test fails and the non-strict alignment test passes; one double away it is the other way round"""
    fz = FROZEN["threshold_equalities"]; st = {t: fz.f["status"][c] for c, t in enumerate(fz.tags)}; prm = {t: fz.f["prm"][c] for c, t in enumerate(fz.tags)}
    for s in ("", "sym_"):
        assert st[s + "map_at_r"][1] != ST_MAPPED and st[s + "map_below_r"][1] == ST_MAPPED
        assert st[s + "aln_at_a"][2] == ST_ALIGNED and st[s + "aln_above_a"][2] == ST_NEWREP
        assert math.nextafter(prm[s + "map_at_r"][3], 0.0) == prm[s + "map_below_r"][3] and math.nextafter(prm[s + "aln_at_a"][4], 1.0) == prm[s + "aln_above_a"][4]
    assert prm["sym_map_at_r"][3] < prm["map_at_r"][3] and prm["sym_aln_at_a"][4] < prm["aln_at_a"][4]      # the representative-side ratio is the smaller one
    base = [c for c, t in enumerate(fz.tags) if t == "base"][0]
    assert prm["map_at_r"][3] == fz.f["tr_ratio"][base][1]      # r is the reference's own trace


@pytest.mark.parametrize("mf", ["mf08", "mf12"])
def test_fraction_boundary_outcomes(oracle, mf):
    """(e) the later founder B shares ceil(f t) - 1 / ceil(f t) / t + 1 minimizers with X: B is not looked at (X founds a cluster), B is visited and takes X, B is the new top
    and takes X.  In all three X fails against A alone (the same reads without B), so a driver that skips the second decision gives another answer."""
    from ngspeciesid_amd.hostutil import subset_reads
    want = ST_MAPPED if mf == "mf08" else ST_ALIGNED
    for which, status, rep in (("below", ST_NEWREP, 2), ("at", want, 1), ("top", want, 1)):
        fz = FROZEN["fraction_boundary_%s_%s" % (which, mf)]
        assert fz.f["status"][0].tolist() == [ST_NEWREP, ST_NEWREP, status] and fz.f["rep_of"][0][2] == rep, which
        prm, kw = fz.call(0)
        mz = CC.minimizers(oracle, [fz.rs.get(i)[0] for i in range(3)])
        t, nb = CC.hits(mz[2], mz[0])[0], CC.hits(mz[2], mz[1])[0]
        c = int(math.ceil(min(prm.min_fraction, 1.0) * t))
        assert nb == {"below": c - 1, "at": c, "top": t + 1}[which] and c - 1 >= prm.min_shared
        st = oracle.cluster_greedy(subset_reads(fz.rs, np.array([0, 2])), prm)[2]
        assert st.tolist() == [ST_NEWREP, ST_NEWREP]


def test_chain_founders_and_word_positions():
    """(f) every read of the chain was compared with its predecessor and founded a cluster; (g) at least 257 new representatives among the first 512 items and joiners behind
    them; (h) new representatives at the word boundaries, the item behind a tentative one affected by it"""
    f = FROZEN["dependent_chain"].f
    assert (f["status"][0] == ST_NEWREP).all() and (f["tr_ns"][0][1:] >= 5).all() and (f["pairs"][0][1:] == 1).all()
    f = FROZEN["many_founders"].f
    assert int((f["status"][0][:512] == ST_NEWREP).sum()) >= 257 and int((f["status"][0][:512] != ST_NEWREP).sum()) >= 20
    assert int((f["status"][0] == ST_NEWREP).sum()) == 600 and (f["status"][0][-60:] != ST_NEWREP).all()
    for n in CC.WORD_COUNTS:
        f = FROZEN["word_boundaries_n%d" % n].f
        new = set(np.nonzero(f["status"][0] == ST_NEWREP)[0].tolist())
        assert {p for p in (0, 63, 64, 127, n - 1) if p < n} <= new, n
        assert new <= {0, 20, 21, 63, 64, 100, 101, 127, n - 1}
        for p in (21, 64, 101):
            if p < n - 1 or (p < n and p == 64): assert f["tr_ns"][0][p] >= 5 and f["tr_best"][0][p] == -1      # shares with the founder in front of it, founds its own cluster
            if p + 1 < n - 1: assert f["rep_of"][0][p + 1] == p


def test_dense_founder_and_merge_round_conditions(oracle):
    """(i) the founder holds more minimizers than the in-LDS sort of a representative takes (25 000 and 16 397 bases) or exactly as many (16 396), and the copies join it;
    (j) the calls differ where they should"""
    for L in CC.DENSE_LENGTHS:
        fz = FROZEN["dense_long_founder_%d" % L]
        moff = oracle.hpc_minimizers(fz.rs, fz.k, fz.w)[0]
        assert int(moff[1]) == L - 12
        assert fz.f["rep_of"][0].tolist() == [0, 1, 0, 0, 4, 0, 0, 7]
    fz = FROZEN["merge_round_edges"]; st = {t: fz.f["status"][c] for c, t in enumerate(fz.tags)}
    assert (st["all_seeded"] == ST_SEEDED).all()
    assert st["mixed"][2] == ST_SEEDED and st["mixed"][9] == ST_SHORT and st["mixed"][10] == ST_NEWREP and st["mixed"][11] == ST_NEWREP
    assert st["mixed"][4] == ST_MAPPED and fz.f["rep_of"][1][4] == 0           # a higher-batch representative re-clustered into a seeded one
    assert st["zeros"][3] == ST_NEWREP and st["zeros"][4] == ST_MAPPED          # batch 0 is processed, not seeded
    assert st["lowest_two"].tolist() == st["mixed"].tolist()
    assert st["mixed"][6] == ST_ALIGNED and st["known_differs"][6] == ST_MAPPED # the known error rate, not the computed one, picks the table row


def test_single_hit_at_either_end(oracle):
    """min_shared = 1: the only hit of read 1 is its first minimizer, of read 2 its last; both were looked at by both stages and founded clusters"""
    fz = FROZEN["single_hit_ends"]; f = fz.f
    mz = CC.minimizers(oracle, [fz.rs.get(i)[0] for i in range(3)])
    assert CC.hits(mz[1], mz[0])[2].tolist() == [0] and CC.hits(mz[2], mz[0])[2].tolist() == [len(mz[2][0]) - 1]
    assert f["tr_ns"][0].tolist()[1:] == [1, 1] and f["pairs"][0].tolist() == [0, 1, 1] and (f["status"][0] == ST_NEWREP).all()
    assert f["tr_ratio"][0][1] > 0 or f["tr_ratio"][0][2] > 0
