"""GPU: the POA tile engine (k_poa.hip) against the independent reference (poa_reference.py) on the families of poa_cases.py - consensus strings, coverage
arrays and the weighted entry point, exactly - on every group whose reference result hung on no tie (`decided`; tests/test_poa_reference_cpu.py asserts
that this is at least 70 % and at least 12 groups of every family, so nothing passes here by being left out).  Routes:
  a  one graph per group (tile_depth = 0), one group per call, the band of the group's shape given explicitly ...
  e  ... and as band <= 0 (the library's default);
  b  tile_depth = 4 with single_below = depth + 1: the route small clusters take by default;
  c  all groups of a family in ONE call, reads stored in shuffled order (lengths interleaved) and reached through read_order;
  d  the one-call route on contexts with poa_host_levels 0 / 1, poa_out_slots 1 and poa_level_budget_mb 1 (include/ngsid.h: results never depend on them).
Expected values are computed once per family and chunk (poa_cases.expected).  Every GPU step runs under a time limit of its own: a step that hangs ends
the process (faulthandler) instead of the next step being started on the same device.
"""
import contextlib, faulthandler, sys
import numpy as np
import pytest
from ngspeciesid_amd._capi import ReadSet, poa_params
import poa_cases as pc

FAMS = sorted(pc.FAMILIES)
STEP_LIMIT = 120      # seconds per library call (they take milliseconds)
OPTIONS = {"host_levels0": {"poa_host_levels": 0}, "host_levels1": {"poa_host_levels": 1}, "out_slots1": {"poa_out_slots": 1}, "budget1mb": {"poa_level_budget_mb": 1}}


@contextlib.contextmanager
def limit(seconds=STEP_LIMIT):
    faulthandler.dump_traceback_later(seconds, exit=True, file=sys.stderr)
    try: yield
    finally: faulthandler.cancel_dump_traceback_later()


def _prm(fam, **kw):
    return poa_params(mode=fam.mode, match=fam.match, mismatch=fam.mismatch, gap=fam.gap, trim=0, **kw)


def _check(what, name, got, want):
    cons, cov = want
    if isinstance(got, tuple):
        assert got[0] == cons, "%s [%s]: consensus (cov call)\n  got      %s\n  expected %s" % (name, what, got[0], cons)
        assert np.array_equal(got[1], cov), "%s [%s]: coverage\n  got      %s\n  expected %s" % (name, what, got[1].tolist(), cov.tolist())
    else:
        assert got == cons, "%s [%s]: consensus\n  got      %s\n  expected %s" % (name, what, got, cons)


def _per_group(api, fam, chunk, what, **kw):
    """one group per call through every entry point that applies; kw(g) -> the route's parameters"""
    n = 0
    for g, (cons, cov, decided) in zip(fam.groups(chunk), pc.expected(fam, chunk)):
        if not decided: continue
        n += 1
        rs = ReadSet.from_strings(g.seqs, g.quals); off = [0, len(g.seqs)]
        for label, k in kw["routes"](g):
            prm = _prm(fam, **k)
            if fam.weighted:
                with limit(): got = api.poa_consensus_weighted(rs, off, prm, g.weights)[0]
                _check("%s %s weighted" % (what, label), g.name, got, (cons, cov))
            else:
                with limit(): got = api.poa_consensus(rs, off, prm)[0]
                _check("%s %s" % (what, label), g.name, got, (cons, cov))
                with limit(): got = api.poa_consensus_cov(rs, off, prm)[0]
                _check("%s %s" % (what, label), g.name, got, (cons, cov))
    assert n > 0


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", pc.CHUNKS)
@pytest.mark.parametrize("family", FAMS)
def test_one_graph_equals_reference(gpu_api, family, chunk):
    """routes a and e"""
    _per_group(gpu_api, pc.FAMILIES[family], chunk, "one graph",
               routes=lambda g: [("band %d" % g.band, dict(tile_depth=0, band=g.band)), ("default band", dict(tile_depth=0, band=0)), ("band -1", dict(tile_depth=0, band=-1))])


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", pc.CHUNKS)
@pytest.mark.parametrize("family", FAMS)
def test_single_below_route_equals_reference(gpu_api, family, chunk):
    """route b: a group with fewer sequences than single_below is one graph in file order whatever tile_depth says"""
    _per_group(gpu_api, pc.FAMILIES[family], chunk, "single_below",
               routes=lambda g: [("depth + 1", dict(tile_depth=4, band=0, single_below=len(g.seqs) + 1)), ("depth + 1, band %d" % g.band, dict(tile_depth=4, band=g.band, single_below=len(g.seqs) + 1))])


_calls = {}


def _family_call(fam):
    """all groups of the family as one call: reads stored in a shuffled order, groups listed in a shuffled order too -> (ReadSet, read_order, grp_off, weights, group permutation)"""
    if fam.name not in _calls:
        gs = fam.all_groups()
        rng = np.random.default_rng([77, fam.fid])
        flat = [(gi, k) for gi, g in enumerate(gs) for k in range(len(g.seqs))]
        store = rng.permutation(len(flat))                               # storage slot x holds read flat[store[x]]
        slot_of = {flat[int(f)]: x for x, f in enumerate(store)}
        fasta = gs[0].quals is None
        rs = ReadSet.from_strings([gs[flat[int(f)][0]].seqs[flat[int(f)][1]] for f in store],
                                  None if fasta else [gs[flat[int(f)][0]].quals[flat[int(f)][1]] for f in store])
        weights = np.array([gs[flat[int(f)][0]].weights[flat[int(f)][1]] for f in store], dtype=np.uint32) if fam.weighted else None
        gperm = [int(x) for x in rng.permutation(len(gs))]
        order, off = [], [0]
        for gi in gperm:
            order += [slot_of[(gi, k)] for k in range(len(gs[gi].seqs))]; off.append(len(order))
        lens = [len(gs[gi].template) for gi in gperm]
        assert any(a > 2 * b for a, b in zip(lens, lens[1:])) and any(b > 2 * a for a, b in zip(lens, lens[1:]))      # short and long groups really alternate
        _calls[fam.name] = (rs, np.array(order, dtype=np.uint32), np.array(off, dtype=np.uint64), weights, gperm)
    return _calls[fam.name]


def _one_call(api, fam, what, **kw):
    rs, order, off, weights, gperm = _family_call(fam)
    gs = fam.all_groups(); exp = [e for c in pc.CHUNKS for e in pc.expected(fam, c)]
    prm = _prm(fam, **kw)
    if fam.weighted:
        with limit(): got = api.poa_consensus_weighted(rs, off, prm, weights, read_order=order)
    else:
        with limit(): got = api.poa_consensus(rs, off, prm, read_order=order)
        with limit(): got_cov = api.poa_consensus_cov(rs, off, prm, read_order=order)
    assert len(got) == len(gperm)
    n = 0
    for x, gi in enumerate(gperm):
        cons, cov, decided = exp[gi]
        if not decided: continue
        n += 1
        _check(what, gs[gi].name, got[x], (cons, cov))
        if not fam.weighted: _check(what, gs[gi].name, got_cov[x], (cons, cov))
    assert n >= 12


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMS)
def test_family_in_one_call_equals_reference(gpu_api, family):
    """route c (the other half, one group per call, is test_one_graph_equals_reference)"""
    fam = pc.FAMILIES[family]
    _one_call(gpu_api, fam, "one call, default band", tile_depth=0, band=0)
    _one_call(gpu_api, fam, "one call, band 128", tile_depth=0, band=128)
    _one_call(gpu_api, fam, "one call, single_below 81", tile_depth=4, band=0, single_below=81)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", sorted(OPTIONS))
@pytest.mark.parametrize("family", FAMS)
def test_context_options_equal_reference(gpu_api, family, setting):
    """route d"""
    from ngspeciesid_amd import runtime
    fam = pc.FAMILIES[family]
    with limit(): api = runtime.new_api(options=OPTIONS[setting])
    try:
        _one_call(api, fam, "one call [%s]" % setting, tile_depth=0, band=0)
        _one_call(api, fam, "one call, single_below [%s]" % setting, tile_depth=4, band=0, single_below=81)
        _per_group(api, fam, "small", "[%s]" % setting, routes=lambda g: [("band %d" % g.band, dict(tile_depth=0, band=g.band))])
    finally:
        with limit(): api.close()
