"""The independent POA reference (poa_reference.py) against the hand-derived vectors and against the CPU oracle, on the families of poa_cases.py.  No GPU.

The oracle (oracle/ngsid_oracle_poa.c) is a restatement that shares band, rank and sibling rules with the kernel; the reference shares nothing with
either and says when its own result hung on a tie (`decided`).  On every decided group the oracle must give the reference's consensus and coverage.
The share of decided groups is asserted HERE, from the reference alone, so that no comparison (this one or the GPU one) can pass by leaving cases out.
"""
import numpy as np
import pytest
from ngspeciesid_amd._capi import ReadSet, poa_params
import poa_cases as pc
import poa_reference as ref
import test_anchor_poa_hand as hand

FAMS = sorted(pc.FAMILIES)
FASTQ_FAMS = [f for f in FAMS if not pc.FAMILIES[f].fasta and not pc.FAMILIES[f].weighted]


@pytest.mark.parametrize("name", sorted(hand.CASES))
def test_reference_reproduces_hand_vectors(name):
    seqs, quals, want = hand.CASES[name]
    assert ref.poa_reference(seqs, quals, None, ref.LOCAL, 5, -4, -2)[0] == want
    if name not in ("fasta_unit_weights", "branch_completion"):
        assert ref.poa_reference(seqs, quals, None, ref.GLOBAL, 3, -5, -4)[0] == want


def test_flag_sees_the_structural_tie():
    """5 / -4 / -2: a novel mismatch (-4) costs exactly two gaps, so "new sibling" and "two unaligned columns" are co-optimal and give different graphs;
    3 / -5 / -4: the mismatch (-5) beats two gaps (-8)"""
    seqs, quals, want = hand.CASES["majority_substitution"]
    assert ref.poa_reference(seqs, quals, None, ref.LOCAL, 5, -4, -2)[2] is False
    assert ref.poa_reference(seqs, quals, None, ref.GLOBAL, 3, -5, -4)[2] is True
    for name in ("majority_insertion", "majority_deletion", "minority_indels"):
        assert ref.poa_reference(*hand.CASES[name][:2], None, ref.LOCAL, 5, -4, -2)[2] is True, name


def _prm(fam, band):
    return poa_params(mode=fam.mode, match=fam.match, mismatch=fam.mismatch, gap=fam.gap, tile_depth=0, band=band, trim=0)


@pytest.mark.parametrize("chunk", pc.CHUNKS)
@pytest.mark.parametrize("family", FAMS)
def test_oracle_equals_reference_on_decided_groups(oracle, family, chunk):
    fam = pc.FAMILIES[family]
    n = 0
    for g, (cons, cov, decided) in zip(fam.groups(chunk), pc.expected(fam, chunk)):
        if not decided: continue
        n += 1
        rs = ReadSet.from_strings(g.seqs, g.quals); off = [0, len(g.seqs)]
        for band in (g.band, 0):
            if fam.weighted:
                assert oracle.poa_consensus_weighted(rs, off, _prm(fam, band), g.weights)[0] == cons, (g.name, band)
            else:
                assert oracle.poa_consensus(rs, off, _prm(fam, band))[0] == cons, (g.name, band)
                c2, v2 = oracle.poa_consensus_cov(rs, off, _prm(fam, band))[0]
                assert c2 == cons, (g.name, band)
                assert np.array_equal(v2, cov), (g.name, band, v2.tolist(), cov.tolist())
    assert n > 0


@pytest.mark.parametrize("family", FAMS)
def test_decided_share_and_sensitivity(family):
    """a CONDITION of the anchor: at least 70 % of a family's groups and at least 12 groups are decided; and the votes matter: in at least 90 % of the
    groups the consensus is not the template"""
    fam = pc.FAMILIES[family]
    gs = fam.all_groups(); exp = [e for c in pc.CHUNKS for e in pc.expected(fam, c)]
    nd = sum(1 for e in exp if e[2])
    print("%s: %d of %d groups decided" % (family, nd, len(gs)))
    assert nd >= 12 and nd >= 0.7 * len(gs), (family, nd, len(gs))
    differs = sum(1 for g, e in zip(gs, exp) if e[0] != g.template)
    assert differs >= 0.9 * len(gs), (family, differs, len(gs))


@pytest.mark.parametrize("family", FASTQ_FAMS)
def test_weights_matter(family):
    """with unit weights instead of the qualities at least one consensus of the family changes"""
    fam = pc.FAMILIES[family]
    for chunk in ("small", "mid"):
        for g, e in zip(fam.groups(chunk), pc.expected(fam, chunk)):
            if ref.poa_reference(g.seqs, None, None, fam.mode, fam.match, fam.mismatch, fam.gap)[0] != e[0]: return
    pytest.fail("%s: no consensus depends on the qualities" % family)


def test_generator_rules():
    """what poa_cases.py promises: templates without equal neighbours, shapes of every band edge and depth, nodes with three and four in-edges"""
    lens, depths = set(), set()
    for fam in pc.FAMILIES.values():
        for g in fam.all_groups():
            assert all(a != b for a, b in zip(g.template, g.template[1:])), g.name
            assert g.seqs[0] and (fam.clipped or all(abs(len(s) - len(g.template)) < len(g.template) // 4 for s in g.seqs))
            lens.add(len(g.template)); depths.add(len(g.seqs))
            if fam.weighted: assert g.quals is None and len(g.weights) == len(g.seqs)
    assert lens >= {63, 64, 65, 127, 128, 129, 255, 257, 400, 1000, 150} and depths >= {2, 3, 5, 10, 24, 40, 80}
    assert sum(1 for fam in pc.FAMILIES.values() for g in fam.all_groups() if len(g.template) == 1000 and len(g.seqs) >= 40) <= 2
    fam = pc.FAMILIES["global_354_all"]; g = fam.groups("mid")[5]
    G = ref.Graph()
    for k, s in enumerate(g.seqs):
        s = s.encode()
        G.add_sequence(s, ref.base_weights(len(s), g.quals[k]), ref.align(G, s, fam.mode, fam.match, fam.mismatch, fam.gap)[0] if G.letter else {})
    indeg = {len(d) for d in G.inn}
    assert 3 in indeg and 4 in indeg, indeg
