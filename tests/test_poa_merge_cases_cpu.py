"""The groups of poa_merge_cases.py: the reference decides each without a tie, and each sits on the route of the merge (k_poa.hip, MergeLds) it was built for.
The routes are checked from the read lengths alone, so a change to the generator cannot quietly move a group off its route: merging read 1 into the graph of
read 0 (V = len(read 0) nodes) makes at least len(read 1) - len(read 0) new nodes, since at most V positions can be aligned."""
import poa_merge_cases as mc


def test_lengths_are_the_documented_ones():
    assert [tuple(len(s) for s in g.seqs) for g in mc.groups()] == mc.LENGTHS
    assert [g.band for g in mc.groups()] == [64, 128, 256, 128]


def test_reference_decides_every_group():
    for g, (cons, cov, decided) in zip(mc.groups(), mc.expected()):
        assert decided, g.name
        assert len(cons) == len(cov) and len(cons) > 0, g.name


def test_capacity_rule_is_not_hit():
    """a graph that would grow beyond max(1.75 * first, longest + 1) nodes is split (oracle g_add_alignment).  The nodes of a group are the columns of its template
    plus one per inserted-base site (sites are at least n / 12 apart on average: well under 60 of them)"""
    for g, (n, depth, cut, band) in zip(mc.groups(), mc.SHAPES):
        first, longest = len(g.seqs[0]), max(len(s) for s in g.seqs)
        assert n + 60 < max(first * 28 // 16, longest + 1), g.name


def test_edge_capacity_splits_group2_at_the_default_only():
    """the edge half of the capacity rule, from the lengths: a graph of reads 0 and 1 has at least first - 1 + (len(read 1) - first) edges"""
    for g in mc.groups():
        first = len(g.seqs[0]); capv = max(first * 28 // 16, first + 64, max(len(s) for s in g.seqs) + 1)
        assert (len(g.seqs[1]) - 1 + len(g.seqs[2]) > 3 * capv // 2) == (g is mc.groups()[2]), g.name
    g = mc.groups()[2]; first = len(g.seqs[0])
    assert mc.NODE_CAP[2] == 40 and mc.SHAPES[2][0] + 120 + len(g.seqs[2]) <= 3 * (first * 40 // 16) // 2      # nodes + 120 bounds the edges: room for the third read


def test_oracle_equals_reference_when_the_graph_is_not_split(oracle):
    """the CPU restatement of the engine, at the bands of the GPU test: with NODE_CAP no group meets the capacity rule, and no band is too narrow for its overhang"""
    from ngspeciesid_amd._capi import ReadSet, poa_params
    fam = mc.FAMILY
    for g, nc, (cons, cov, decided) in zip(mc.groups(), mc.NODE_CAP, mc.expected()):
        for band in sorted({g.band, 64}):
            prm = poa_params(mode=fam.mode, match=fam.match, mismatch=fam.mismatch, gap=fam.gap, trim=0, tile_depth=0, band=band, node_cap=nc)
            got = oracle.poa_consensus_cov(ReadSet.from_strings(g.seqs, g.quals), [0, len(g.seqs)], prm)[0]
            assert got[0] == cons and list(got[1]) == list(cov), (g.name, band)


def test_group0_takes_the_hbm_route_at_band_64():
    g = mc.groups()[0]
    for s in g.seqs[1:]:
        assert 2 * len(s) > mc.TBR * 64 and not mc.seq_lds(len(s), 64)
        assert mc.nn_cap(len(s), 64) == 0 and not mc.sh_lds(len(s), len(g.seqs[0]), 1, 64)


def test_group1_shift_in_lds_records_by_the_chunk_walk():
    g = mc.groups()[1]; L, V = len(g.seqs[1]), len(g.seqs[0]); d = L - V
    assert mc.seq_lds(L, 128) and 2 * L <= mc.TBR * 128
    assert mc.nn_cap(L, 128) == 196 and mc.nn_cap(L, 128) < d <= 255 - 30      # (30: room for the inserted bases and mismatches of the overlap)
    assert mc.sh_lds(L, V, 255, 128) and not mc.nn_lds(L, d, 128)


def test_group2_shift_in_hbm_records_from_the_list():
    g = mc.groups()[2]; L, V = len(g.seqs[1]), len(g.seqs[0]); d = L - V
    assert mc.seq_lds(L, 256) and 2 * L <= mc.TBR * 256
    assert mc.nn_cap(L, 256) == 808 and 255 < d and d + 60 <= mc.nn_cap(L, 256)      # (60: room for the inserted bases and mismatches of the overlap)
    assert not mc.sh_lds(L, V, d, 256) and mc.nn_lds(L, d, 256) and mc.nn_lds(L, d + 60, 256)


def test_group3_both_fall_backs_and_all_hbm_at_band_64():
    g = mc.groups()[3]; L, V = len(g.seqs[1]), len(g.seqs[0]); d = L - V
    assert mc.seq_lds(L, 128) and 2 * L <= mc.TBR * 128
    assert 255 < d and mc.nn_cap(L, 128) < d
    assert not mc.sh_lds(L, V, d, 128) and not mc.nn_lds(L, d, 128)
    assert 2 * L > mc.TBR * 64 and not mc.seq_lds(L, 64)


def test_predicates_at_their_thresholds():
    """the plain-Python mirror at the sizes where a route changes (band 64 / 128 / 256): 2 L against the direction block, the chunk summaries against the row-info block"""
    assert mc.seq_lds(1024, 64) and not mc.seq_lds(1025, 64)
    assert mc.seq_lds(1344, 128) and not mc.seq_lds(1345, 128)       # 21 chunks of 12 bytes fit 256, 22 do not
    assert mc.seq_lds(1344, 256) and not mc.seq_lds(1345, 256)
    assert mc.sh_lds(1000, 2560 - 2000 - 2, 255, 64) and not mc.sh_lds(1000, 2560 - 2000 - 1, 255, 64) and not mc.sh_lds(1000, 10, 256, 64)
    assert mc.nn_cap(1000, 64) == 6 and mc.nn_cap(1001, 64) == 4 and mc.nn_cap(1025, 64) == 0
    assert mc.nn_lds(1000, 6, 64) and not mc.nn_lds(1000, 7, 64) and not mc.nn_lds(1000, 0, 64)
