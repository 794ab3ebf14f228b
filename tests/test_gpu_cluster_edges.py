"""The adversarial clustering cases (tests/cluster_cases.py, frozen in tests/golden/cluster_edges.npz) on the GPU: the block driver of csrc/k_cluster.hip gives what the
reference's reads_to_clusters and the oracle's sequential loop give - membership, status, counters, HPC error rates bit-equal to the oracle's - whatever the block size and
wherever restarting blocks are cut."""
import numpy as np
import pytest
import cluster_cases as CC
from ngspeciesid_amd._capi import NgsidError, ReadSet, cluster_params

pytestmark = pytest.mark.gpu
FROZEN = {f.name: f for f in CC.load_frozen()}
ST_MAPPED, ERR_NO_PTABLE = 1, -7
SETTINGS = [{}, {"cluster_block": 64}, {"cluster_block": 128}] + [{"cluster_block": 64, "cluster_trunc": t} for t in (1, 63, 64, 65)]
REGROW = {"cluster_block": 512}          # many_founders: more than 256 new representatives inside one block


@pytest.fixture(scope="module")
def contexts(gpu_api):
    """one context per driver setting (the shared context serves the default and keeps its options), closed when the module is done"""
    from ngspeciesid_amd import runtime
    made = {}

    def get(opts):
        key = tuple(sorted(opts.items()))
        if not key: return gpu_api
        if key not in made: made[key] = runtime.new_api(options=dict(opts))
        return made[key]
    yield get
    for api in made.values(): api.close()


_expected = {}


def expected(oracle, fz, c):
    """the oracle's result of call c, computed once"""
    if (fz.name, c) not in _expected:
        prm, kw = fz.call(c)
        _expected[(fz.name, c)] = oracle.cluster_greedy(fz.rs, prm, **kw)
    return _expected[(fz.name, c)]


@pytest.mark.parametrize("name", sorted(FROZEN))
def test_hip_equals_fixture_and_oracle(contexts, oracle, name):
    fz = FROZEN[name]; f = fz.f
    for opts in SETTINGS + ([REGROW] if name == "many_founders" else []):
        api = contexts(opts)
        for c, tag in enumerate(fz.tags):
            prm, kw = fz.call(c)
            rep, herr, st, cnt = api.cluster_greedy(fz.rs, prm, **kw)
            orep, oherr, ost, ocnt = expected(oracle, fz, c)
            where = (name, tag, opts)
            assert np.array_equal(rep, f["rep_of"][c]) and np.array_equal(st, f["status"][c]), (where, np.nonzero((rep != f["rep_of"][c]) | (st != f["status"][c]))[0][:10])
            assert [int(x) for x in cnt[:3]] == [int(x) for x in f["counters"][c]], where
            assert np.array_equal(rep, orep) and np.array_equal(st, ost) and np.array_equal(cnt, ocnt), where
            assert np.array_equal(herr, oherr, equal_nan=True), where


def test_round2_cells_are_told_apart(gpu_api):
    """(a) the table of a call holds another value one row / column beside the expected cell and NaN in the transposed one: with the neighbour's value in the expected cell
    the pair no longer maps, with the table transposed the call fails with NGSID_ERR_NO_PTABLE - so the statuses of test_hip_equals_fixture_and_oracle pin the cell"""
    fz = FROZEN["round2_boundaries"]
    for c in (5, 20, 60, 90):
        prm, kw = fz.call(c)
        t = CC.round2_table(kw["known_err"][1], kw["known_err"][0]).reshape(15, 15)
        i, j = CC.round2_index(kw["known_err"][1]), CC.round2_index(kw["known_err"][0])
        shifted = t.copy(); shifted[i - 1, j - 1] = 1.0
        assert gpu_api.cluster_greedy(fz.rs, cluster_params(k=13, w=20, p_shared=shifted.reshape(225)), **kw)[2][1] != ST_MAPPED
        with pytest.raises(NgsidError) as ei:
            gpu_api.cluster_greedy(fz.rs, cluster_params(k=13, w=20, p_shared=t.T.copy().reshape(225)), **kw)
        assert ei.value.code == ERR_NO_PTABLE
        assert gpu_api.cluster_greedy(fz.rs, prm, **kw)[2][1] == ST_MAPPED          # the context works on after the error


@pytest.mark.parametrize("name", sorted(n for n in FROZEN if not n.startswith("dense_")))
def test_segmented_call_equals_the_plain_call(contexts, oracle, name):
    """the same reads twice as two segments of cluster_greedy_segmented: each segment equals the plain call (the fixture, for the calls without prev_batch / known_err, which the
    segmented call does not take; the oracle's plain default call for the reads of the cases that only have merge-round calls)"""
    fz = FROZEN[name]; n = fz.rs.n
    seqs = [fz.rs.get(i)[0] for i in range(n)]; quals = [fz.rs.get(i)[1] for i in range(n)]
    two = ReadSet.from_strings(seqs + seqs, quals + quals); ar = np.concatenate([fz.acc_rank, fz.acc_rank])
    plain = [c for c in range(len(fz.tags)) if not fz.f["has_prev"][c] and not fz.f["has_known"][c]]
    for c in plain or [None]:
        if c is None:
            from ngspeciesid_amd.ptable import select_p_table
            prm = cluster_params(k=fz.k, w=fz.w, p_shared=select_p_table(fz.k, fz.w))
            rep1, herr1, st1, cnt1 = oracle.cluster_greedy(fz.rs, prm, acc_rank=fz.acc_rank)
        else:
            prm, _ = fz.call(c)
            rep1, herr1, st1, cnt1 = expected(oracle, fz, c)
            assert np.array_equal(rep1, fz.f["rep_of"][c])
        for opts in ({}, {"cluster_block": 64, "cluster_trunc": 1}):
            rep, herr, st, cnt = contexts(opts).cluster_greedy_segmented(two, prm, [0, n, 2 * n], acc_rank=ar)
            for s in (0, 1):
                sl = slice(s * n, (s + 1) * n)
                assert np.array_equal(rep[sl], rep1 + s * n) and np.array_equal(st[sl], st1) and np.array_equal(herr[sl], herr1, equal_nan=True), (name, c, opts, s)
                assert np.array_equal(cnt[s], cnt1), (name, c, opts, s)
