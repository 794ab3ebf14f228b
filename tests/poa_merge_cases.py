"""Four POA groups that reach the fall-back routes of the merge in k_poa.hip (struct MergeLds), which no group of poa_cases.py does: its longest read is 1 000
bases at band 128 and its largest overhang 25 bases.  Used by tests/test_poa_merge_cases_cpu.py (the preconditions, from the lengths alone) and
tests/test_gpu_poa_merge_paths.py (the engine against poa_reference.py).

The first read of every group is cut by `cut` bases at each end, so the later reads hang over the graph by more than a hundred bases per end: that many NEW nodes
in one alignment.  Routes (L = length of the read being merged, V = nodes of the graph, nnew = new nodes of the alignment):
  seq   alnode[] / nodeof[] in LDS: 2 L fits the DP ring and the direction block, the chunk summaries fit the row-info block
  sh    shift[] in LDS: seq, nnew <= 255, and V + 2 bytes fit the ring behind alnode[]
  nn    the new-node list in LDS: 0 < nnew <= nn_cap = what the direction block has left behind nodeof[], in entries of 8 bytes
"""
import poa_cases as pc

FAMILY = pc.Family(101, "local_542", pc.LOCAL, (5, -4, -2), pc.INDELS, clipped=True)

# constants of ngspeciesid_amd/csrc/k_poa.hip, copied: DP rows in the LDS ring, guard cells left / right of a ring row, direction rows per traceback block
HR, RPADL, RPADR, TBR = 8, 4, 12, 32


def ring_bytes(bw): return HR * (bw + RPADL + RPADR) * 4
def dir_bytes(bw): return TBR * bw
def rblk_bytes(): return TBR * 8
def seq_end(L): return 2 * ((L + 7) & ~7)


# the three predicates of MergeLds, in plain Python
def seq_lds(L, bw): return 2 * L <= ring_bytes(bw) and 2 * L <= dir_bytes(bw) and 12 * ((L + 63) // 64) <= rblk_bytes()
def sh_lds(L, V, nnew, bw): return seq_lds(L, bw) and nnew <= 255 and seq_end(L) + V + 2 <= ring_bytes(bw)
def nn_cap(L, bw): return (dir_bytes(bw) - seq_end(L)) // 8 if seq_lds(L, bw) else 0
def nn_lds(L, nnew, bw): return 0 < nnew <= nn_cap(L, bw)


#         n, depth, cut, band of the route
SHAPES = [(1100, 3, 0, 64),       # band 64: 2 L > TBR * BW, seq false: everything through HBM
          (1300, 3, 125, 128),    # band 128: seq; nnew <= 255 but above nn_cap: sh true, nn false (the chunk walk writes the records)
          (900, 3, 160, 256),     # band 256: nnew above 255 and within nn_cap: sh false, nn true
          (1300, 3, 150, 128)]    # band 128: nnew above 255 and above nn_cap: both fall-backs with seq true.  Band 64: all HBM
LENGTHS = [(1104, 1084, 1072), (1049, 1264, 1267), (581, 863, 883), (996, 1266, 1288)]      # what the generator gives (asserted by the CPU test)
# The engine splits a graph that would outgrow its capacity (oracle g_add_alignment: V + nnew > capV or E + L > capE, capV = max(first * node_cap / 16, first + 64,
# longest + 1), capE = 3 capV / 2, node_cap 28 by default); the reference knows no such rule.  The NODE half is far away in all four groups.  The EDGE half is hit by
# group 2 at the default: capV = 581 * 28 / 16 = 1016, capE = 1524, and after the second read the graph holds at least 580 + 282 edges, so the third read (883 bases)
# does not fit.  node_cap = 40 (capV 1452, capE 2178) keeps group 2 one graph.
NODE_CAP = [0, 0, 40, 0]

_groups = []


def groups():
    if not _groups:
        for i, (n, depth, cut, band) in enumerate(SHAPES):
            g = pc.make_group(FAMILY, 900 + i, n, depth, 64)
            if cut:
                g.seqs[0] = g.seqs[0][cut:len(g.seqs[0]) - cut]; g.quals[0] = g.quals[0][cut:len(g.quals[0]) - cut]
            g.band = band
            _groups.append(g)
    return _groups


_expected = []


def expected():
    """[(consensus, cov, decided)] by the reference, computed once"""
    if not _expected:
        _expected.extend(pc.ref.poa_reference(g.seqs, g.quals, g.weights, FAMILY.mode, FAMILY.match, FAMILY.mismatch, FAMILY.gap) for g in groups())
    return _expected
