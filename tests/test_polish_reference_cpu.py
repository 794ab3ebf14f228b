"""The independent whole-call reference of the polisher (polish_reference.py) against the CPU oracle, on the families of polish_cases.py.  No GPU.

The oracle's polish_impl was written by the same hand as the library's host code, from the same reading of racon; the reference is written from include/ngsid.h
and stands on ed_reference.py and poa_reference.py only.  On every group whose reference result hung on no tie (`decided`) the oracle must return the reference's
sequences after every iteration, n_used and PAF records.  The decided share is asserted HERE, from the reference alone, so that no comparison (this one or the GPU
one) passes by leaving cases out; and two oracle switches that change a rule show that the comparison can fail.
"""
import ctypes
import numpy as np
import pytest
from ngspeciesid_amd._capi import ReadSet, polish_params
import polish_cases as pc
import polish_reference as ref


def _call(backend, groups, prm, fn, shuffle_seed=None):
    """one call over `groups` -> per group (in the order of `groups`) (seqs[it], used[it], aln[it] or None)"""
    bbs, reads, quals, order, off, listed = pc.pack(groups, shuffle_seed)
    bb = ReadSet.from_strings(bbs); rs = ReadSet.from_strings(reads, quals)
    out = [None] * len(groups)
    if fn == "polish":
        seqs, used = backend.polish(bb, rs, off, prm, read_order=order)
        for x, gi in enumerate(listed): out[gi] = ([seqs[x]], [used[x]], None)
        return out
    r = backend.polish_trace(bb, rs, off, prm, read_order=order, aln=(fn == "polish_trace_aln"))
    for x, gi in enumerate(listed):
        a = None
        if fn == "polish_trace_aln": a = [np.asarray(r[2][it])[int(off[x]):int(off[x + 1])] for it in range(prm.iters)]
        out[gi] = ([r[0][it][x] for it in range(prm.iters)], [r[1][it][x] for it in range(prm.iters)], a)
    return out


def _prm(g, **kw):
    return polish_params(**dict(dict(tile_depth=0, band=0, stop_when_stable=0), **g.prm, **kw))


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_decided_share(family):
    """a CONDITION of the anchor: at least 70 % and at least 8 groups of every family are decided - the reference's own verdict, formed before any other output exists"""
    ex = pc.expected(family)
    nd = sum(1 for e in ex if e[3])
    print("%s: %d of %d groups decided" % (family, nd, len(ex)))
    assert nd >= 8 and nd >= 0.7 * len(ex), (family, nd, len(ex))


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_oracle_equals_reference_one_group_per_call(oracle, family):
    n = 0
    for g, e in zip(pc.family(family), pc.expected(family)):
        if not e[3]: continue
        n += 1
        got = _call(oracle, [g], _prm(g), "polish_trace_aln")[0]
        d = pc.differences(e, *got)
        assert not d, "%s [trace_aln]: %s" % (g.name, "\n".join(d))
        got = _call(oracle, [g], _prm(g), "polish")[0]
        d = pc.differences(e, *got, last_only=True)
        assert not d, "%s [polish]: %s" % (g.name, "\n".join(d))
    assert n >= 8


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_oracle_equals_reference_family_in_one_call(oracle, family):
    """all groups of a family that share their parameters in ONE call"""
    gs = pc.family(family); ex = pc.expected(family)
    n = 0
    for key, idx in pc.call_keys(family):
        groups = [gs[x] for x in idx]
        got = _call(oracle, groups, _prm(groups[0]), "polish_trace_aln")
        last = _call(oracle, groups, _prm(groups[0]), "polish")
        for x, r, l in zip(idx, got, last):
            if not ex[x][3]: continue
            n += 1
            d = pc.differences(ex[x], *r) + pc.differences(ex[x], *l, last_only=True)
            assert not d, "%s [one call]: %s" % (gs[x].name, "\n".join(d))
    assert n >= 8


def test_stop_when_stable_changes_nothing(oracle):
    """the polisher is a function of (backbone, reads): the reference does not model the switch, the oracle must not depend on it"""
    for g in pc.family("f_iterations"):
        assert _call(oracle, [g], _prm(g, stop_when_stable=1), "polish_trace")[0][:2] == _call(oracle, [g], _prm(g, stop_when_stable=0), "polish_trace")[0][:2], g.name


def _differing(oracle, rules, aln_mode=None):
    """decided groups of family b (aln_mode 2 variant) on which the oracle under `rules` differs from the reference"""
    out = []
    oracle.lib.ongsid_debug_polish_rules(ctypes.c_int32(rules))
    try:
        for g, e in zip(pc.family("b_edges"), pc.expected("b_edges")):
            if not e[3] or g.prm["aln_mode"] != 2: continue
            kw = {} if aln_mode is None else {"aln_mode": aln_mode}
            prm = polish_params(**dict(dict(tile_depth=0, band=0, stop_when_stable=0), **dict(g.prm, **kw)))
            if pc.differences(e, *_call(oracle, [g], prm, "polish_trace_aln")[0]): out.append(g.name)
    finally:
        oracle.lib.ongsid_debug_polish_rules(ctypes.c_int32(0))
    return out


def test_comparison_can_fail(oracle):
    """sensitivity: with a rule changed the oracle must DIFFER from the reference on family b - bit 2 (layer ends that the alignment leaves outside the graph create no
    nodes) and bit 0 under aln_mode 1 (overlap-span clipping where the contract has none); with the switches off, aln_mode 1 is aln_mode 2"""
    assert _differing(oracle, 4), "rules bit 2 changed nothing"
    assert _differing(oracle, 1, aln_mode=1), "rules bit 0 changed nothing under aln_mode 1"
    assert not _differing(oracle, 0, aln_mode=1)
    assert oracle.lib.ongsid_debug_polish_rules(ctypes.c_int32(-1)) == 0


def test_subgraph_layers_oracle_equals_reference(oracle):
    """NGSID_ALN_SUBGRAPH as the header defines it, on family b: the oracle under rules bit 1 (with aln_mode 3 also bit 0: the same clipping) equals the reference with
    sub-graph layers on every group the reference calls decided.  In this family the rule changes no decided result (printed): the layers' ends sit at least 7 bases
    from any variant, so end-free and sub-graph alignment agree - what is pinned is that the rule's own path reproduces the window-edge cases, not that it matters
    (tests/test_gpu_polish_subgraph.py has data on which it does)."""
    gs = pc.family("b_edges"); ex = pc.expected("b_edges", subgraph=True); plain = pc.expected("b_edges")
    n = 0
    for g, e in zip(gs, ex):
        if not e[3]: continue
        n += 1
        oracle.lib.ongsid_debug_polish_rules(ctypes.c_int32(3 if g.prm["aln_mode"] == 3 else 2))
        try: got = _call(oracle, [g], _prm(g), "polish_trace_aln")[0]
        finally: oracle.lib.ongsid_debug_polish_rules(ctypes.c_int32(0))
        d = pc.differences(e, *got)
        assert not d, "%s [sub-graph layers]: %s" % (g.name, "\n".join(d))
    print("sub-graph layers: %d of %d groups decided, %d differ from the plain rule" % (n, len(gs), sum(1 for a, b in zip(ex, plain) if a[0] != b[0] and a[3] and b[3])))
    assert n >= 8 and n >= 0.7 * len(gs)


def test_one_call_mixes_short_and_long_backbones():
    """what the one-call route of tests/test_gpu_polish_reference.py promises about its shuffled listing, on the families whose backbones differ in length"""
    for family in ("a_geometry", "d_strands"):
        gs = pc.family(family)
        for k, (key, idx) in enumerate(pc.call_keys(family)):
            if len(idx) < 6: continue
            listed = pc.pack([gs[x] for x in idx], shuffle_seed=100 * k + len(idx))[5]
            lens = [len(gs[idx[x]].backbone) for x in listed]
            assert any(a > 1.5 * b for a, b in zip(lens, lens[1:])) and any(b > 1.5 * a for a, b in zip(lens, lens[1:])), (family, lens)
            assert listed != sorted(listed)


def test_window_geometry():
    """nwin / wlen against a brute-force listing of the windows"""
    for W in (100, 200, 500):
        for Bl in range(1, 1301):
            wins = [min(W, Bl - s) for s in range(0, Bl, W)]
            if len(wins) >= 2 and wins[-1] < W // 10:
                tail = wins.pop(); wins[-1] += tail
            assert ref.nwin(Bl, W) == len(wins), (Bl, W)
            assert [ref.wlen(Bl, W, w) for w in range(len(wins))] == wins, (Bl, W)


def test_minimizer_step_by_hand():
    """k = 3, w = 5 on ACGGTTACAAC: compressed ACGTACAC, k-mers ACG CGT GTA TAC ACA CAC, three per window -> ACG, then GTA's window (CGT GTA TAC) gives CGT, then
    (GTA TAC ACA) ACA, then (TAC ACA CAC) ACA again at the same position: not emitted twice"""
    assert ref.hpc("ACGGTTACAAC") == "ACGTACAC"
    assert ref.minimizers("ACGGTTACAAC", 3, 5) == ["ACG", "CGT", "ACA"]
    assert ref.minimizers("AC", 3, 5) == []                                   # shorter than k after compression
    assert ref.minimizers("ACGT", 3, 7) == [""]                               # fewer k-mers than a window holds: slices past the end take part and the empty one sorts first
    assert ref.revcomp("ACGTN") == "NACGT"


def test_cases_exercise_every_boundary():
    """polish_cases.py's promise (h), read off the reference's `info`: both layer modes, every drop reason, merged and unmerged tails, a window count that changes between
    iterations, both strands and unused reads, TGS on and off, trimming that removes bases, planted backbone errors that the reads correct"""
    count = {}
    for fam in pc.FAMILIES:
        c = count[fam] = {}
        def add(k, n=1): c[k] = c.get(k, 0) + n
        for g, e in zip(pc.family(fam), pc.expected(fam)):
            info = e[4]
            for l in info["layers"]:
                add(("GLOBAL" if l[7] == ref.GLOBAL else "SEMI") + " " + l[8])
                if l[8] != "short" and l[4] - l[3] + 1 == 4: add("layer of 4 bases kept")
                if l[8] == "short" and l[4] - l[3] + 1 == 3: add("layer of 3 bases dropped")
                if l[7] == ref.SEMI and l[5] == 2: add("begin == 2 (SEMI)")
                if l[7] == ref.GLOBAL and l[5] == 1: add("begin == 1 (GLOBAL)")
                if l[7] == ref.SEMI and l[5] == 0 and l[6] == ref.wlen(len(g.backbone), g.prm["window"], l[2]) - 2 and l[0] == 0: add("end == wlen - 2 (SEMI)")
            add("span dropped", len(info["span_dropped"])); add("span ratio exactly 0.7 dropped", sum(1 for s in info["span_dropped"] if s[2] * 10 == s[3] * 7))
            add("unclipped", len(info["unclipped"]))
            for a, b, st in info["reads"]:
                add({0: "plus", 1: "minus", -1: "unused"}[st])
                if a == b and a > 0: add("a == b > 0")
            add("tgs" if info["tgs"] else "not tgs")
            if g.quals is not None:
                for l in info["layers"]:
                    q = g.quals[l[1]]; q = q[::-1] if info["reads"][l[1]][2] == 1 else q
                    margin = sum(ord(x) - 33 for x in q[l[3]:l[4] + 1]) - 10 * (l[4] - l[3] + 1)
                    if margin in (-1, 0, 1) and l[8] != "short": add("quality sum 10 len %+d %s" % (margin, "dropped" if l[8] == "quality" else "kept"))
            if fam == "e_trim":
                assert any(w[3] + w[4] > 0 for w in info["windows"]) == (g.prm["trim"] == 2 or (g.prm["trim"] in (1, 3) and info["tgs"])), g.name
                assert sum(len(r) for r in g.reads) == (3003 if info["tgs"] else 3000), g.name
            add("trimmed windows", sum(1 for w in info["windows"] if w[3] + w[4] > 0))
            add("windows under 2 layers", sum(1 for w in info["windows"] if w[2] < 2))
            if len(set(info["nwin"])) > 1: add("window count changes")
            Bl, W = len(g.backbone), g.prm["window"]
            if Bl > W and Bl % W and Bl % W < W // 10: add("merged tail")
            if Bl > W and Bl % W >= W // 10: add("unmerged tail")
            if e[0][-1] != g.backbone: add("backbone changed")
            if e[3]: add("decided")
            add("groups")
        print(fam, sorted(c.items()))
    a, b, c, d, e, f = (count[x] for x in pc.FAMILIES)
    assert a["merged tail"] >= 2 and a["unmerged tail"] >= 4 and a["backbone changed"] == a["groups"] and a["GLOBAL kept"] and a["SEMI kept"]
    for k in ("GLOBAL kept", "SEMI kept", "SEMI short", "layer of 4 bases kept", "layer of 3 bases dropped", "begin == 2 (SEMI)", "begin == 1 (GLOBAL)", "end == wlen - 2 (SEMI)"): assert b.get(k), k
    for k in ("GLOBAL quality", "span dropped", "span ratio exactly 0.7 dropped", "quality sum 10 len +0 kept", "quality sum 10 len -1 dropped", "quality sum 10 len +1 kept"): assert c.get(k), k
    assert not c.get("quality sum 10 len +0 dropped") and not c.get("quality sum 10 len -1 kept")
    for k in ("plus", "minus", "unused", "windows under 2 layers", "a == b > 0"): assert d.get(k), k
    assert e["tgs"] and e["not tgs"] and e["trimmed windows"]
    assert f["window count changes"] >= 3
