"""GPU: the fall-back routes of the POA merge (k_poa.hip, MergeLds: per-position arrays in the HBM scratch, shift[] in HBM, new-node records written by the chunk
walk) against the independent reference, on the groups of poa_merge_cases.py.  One graph per group (tile_depth = 0), at the band that puts the group on its route
and at 64; consensus strings and coverage arrays must be equal exactly.  tests/test_poa_merge_cases_cpu.py asserts that every group is decided and on its route.
Every GPU step runs under a time limit of its own, as in test_gpu_poa_reference.py.

The reference builds ONE graph and knows no capacity rule, so a group can only equal it while the engine does not split the graph.  Group 2 runs with
node_cap = 40 for that (poa_merge_cases.NODE_CAP): at the default its third read meets the edge half of the rule (at least 862 edges + 883 bases > capE = 1 524),
the graph is split, and engine and CPU oracle alike return 883 bases where the reference has 885 (the bases at positions 47 and 119 are missing)."""
import numpy as np
import pytest
from ngspeciesid_amd._capi import ReadSet, poa_params
import poa_merge_cases as mc
from test_gpu_poa_reference import _check, limit


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(mc.SHAPES)))
def test_merge_route_equals_reference(gpu_api, index):
    g = mc.groups()[index]; cons, cov, decided = mc.expected()[index]; fam = mc.FAMILY
    assert decided, g.name
    rs = ReadSet.from_strings(g.seqs, g.quals); off = [0, len(g.seqs)]
    for band in sorted({g.band, 64}):
        prm = poa_params(mode=fam.mode, match=fam.match, mismatch=fam.mismatch, gap=fam.gap, trim=0, tile_depth=0, band=band, node_cap=mc.NODE_CAP[index])
        with limit(): got = gpu_api.poa_consensus(rs, off, prm)[0]
        _check("merge route, band %d" % band, g.name, got, (cons, cov))
        with limit(): got = gpu_api.poa_consensus_cov(rs, off, prm)[0]
        _check("merge route, band %d" % band, g.name, got, (cons, cov))


@pytest.mark.gpu
def test_longest_reads_of_the_64_column_instance(gpu_api):
    """MergeLds<64>::max_len = 25 920 bases: the chunk summaries of the merge (12 bytes per 64 positions from LDS address 0) end 4 bytes below LLT<64>::C1, where the
    sequence bytes' region starts.  Two equal reads: their consensus is the read (the CPU oracle agrees).  match = 2 keeps match x length below 65 536; node_cap = 22
    keeps the graph capacity within the 16-bit indices and still holds the edges of two reads.  One base more is refused: tests/test_gpu_argument_errors.py."""
    rng = np.random.default_rng(11)
    read = "".join("ACGT"[i] for i in rng.integers(4, size=25920))
    with limit(): got = gpu_api.poa_consensus(ReadSet.from_strings([read, read]), [0, 2], poa_params(match=2, band=64, node_cap=22))[0]
    assert got == read
