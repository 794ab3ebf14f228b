"""GPU: ngsid_polish / ngsid_polish_trace / ngsid_polish_trace_aln against the independent whole-call reference (polish_reference.py) on the families of
polish_cases.py - the sequence after every iteration, n_used and the PAF records, exactly - on every group whose reference result hung on no tie (`decided`;
tests/test_polish_reference_cpu.py asserts that this is at least 70 % and at least 8 groups of every family, so nothing passes here by being left out).  Routes:
  i    one group per call through polish, polish_trace and polish_trace(aln=True), tile_depth = 0, band 0 (the library's default) and 128;
  ii   tile_depth = 4 with single_below = 64: the route small windows take by default;
  iii  all groups of a family that share their parameters in ONE call, reads stored in shuffled order and reached through read_order, groups listed in shuffled
       order (short and long backbones alternate: the launch is sized by the longest, every group indexed by its own length);
  iv   route iii on contexts with poa_host_levels 0 / 1, poa_out_slots 1 and polish_unit_threads 1 / 4 (include/ngsid.h: results never depend on them);
  v    family f (the window count changes between iterations) with stop_when_stable 0 and 1: identical outputs;
  vi   family b under NGSID_ALN_SUBGRAPH against the reference's sub-graph layers, one group per call and all in one call;
  vii  on one polish_unit_threads 4 context (the unit-list builder with as many threads as a large call gives it): route v with all groups in one call (the pairs
       of the stable groups dropped, the pair ranges recomputed), and family d one group per call (groups without a pair, fewer tasks than threads).
Expected values are computed once per family (polish_cases.expected).  Every library call runs under a time limit of its own: a call that hangs ends the process
(faulthandler) instead of the next one being started on the same device.
"""
import contextlib, faulthandler, sys
import numpy as np
import pytest
from ngspeciesid_amd._capi import ReadSet, polish_params
import polish_cases as pc

pytestmark = pytest.mark.gpu
STEP_LIMIT = 120      # seconds per library call (they take milliseconds)
OPTIONS = {"host_levels0": {"poa_host_levels": 0}, "host_levels1": {"poa_host_levels": 1}, "out_slots1": {"poa_out_slots": 1},
           "unit_threads1": {"polish_unit_threads": 1}, "unit_threads4": {"polish_unit_threads": 4}}
MIN_COMPARED = 8


@contextlib.contextmanager
def limit(seconds=STEP_LIMIT):
    faulthandler.dump_traceback_later(seconds, exit=True, file=sys.stderr)
    try: yield
    finally: faulthandler.cancel_dump_traceback_later()


def _prm(g, **kw):
    return polish_params(**dict(dict(tile_depth=0, band=0, stop_when_stable=0), **g.prm, **kw))


def _call(api, groups, prm, fn, shuffle_seed=None):
    """one library call over `groups` -> per group (in the order of `groups`) (seqs[it], used[it], aln[it] or None)"""
    bbs, reads, quals, order, off, listed = pc.pack(groups, shuffle_seed)
    bb = ReadSet.from_strings(bbs); rs = ReadSet.from_strings(reads, quals)
    out = [None] * len(groups)
    if fn == "polish":
        with limit(): seqs, used = api.polish(bb, rs, off, prm, read_order=order)
        for x, gi in enumerate(listed): out[gi] = ([seqs[x]], [used[x]], None)
        return out
    with limit(): r = api.polish_trace(bb, rs, off, prm, read_order=order, aln=(fn == "polish_trace_aln"))
    for x, gi in enumerate(listed):
        a = None
        if fn == "polish_trace_aln": a = [np.asarray(r[2][it])[int(off[x]):int(off[x + 1])] for it in range(prm.iters)]
        out[gi] = ([r[0][it][x] for it in range(prm.iters)], [r[1][it][x] for it in range(prm.iters)], a)
    return out


def _per_group(api, family, what, **kw):
    n = 0
    for g, e in zip(pc.family(family), pc.expected(family)):
        if not e[3]: continue
        n += 1
        for fn in ("polish", "polish_trace", "polish_trace_aln"):
            d = pc.differences(e, *_call(api, [g], _prm(g, **kw), fn)[0], last_only=(fn == "polish"))
            assert not d, "%s [%s, %s]: %s" % (g.name, what, fn, "\n".join(d))
    assert n >= MIN_COMPARED


def _one_call(api, family, what, **kw):
    gs = pc.family(family); ex = pc.expected(family)
    n = 0
    for k, (key, idx) in enumerate(pc.call_keys(family)):
        groups = [gs[x] for x in idx]
        for fn in ("polish_trace_aln", "polish"):
            got = _call(api, groups, _prm(groups[0], **kw), fn, shuffle_seed=100 * k + len(idx))
            for x, r in zip(idx, got):
                if not ex[x][3]: continue
                n += fn == "polish"
                d = pc.differences(ex[x], *r, last_only=(fn == "polish"))
                assert not d, "%s [%s, %s]: %s" % (gs[x].name, what, fn, "\n".join(d))
    assert n >= MIN_COMPARED


@pytest.mark.parametrize("band", [0, 128])
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_one_group_per_call_equals_reference(gpu_api, family, band):
    """route i"""
    _per_group(gpu_api, family, "one graph, band %d" % band, tile_depth=0, band=band)


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_single_below_route_equals_reference(gpu_api, family):
    """route ii: a window with fewer layers than single_below is one graph in racon's order whatever tile_depth says"""
    _per_group(gpu_api, family, "tile_depth 4, single_below 64", tile_depth=4, band=0, single_below=64)


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_family_in_one_call_equals_reference(gpu_api, family):
    """route iii"""
    _one_call(gpu_api, family, "one call", tile_depth=0, band=0)
    _one_call(gpu_api, family, "one call, single_below 64", tile_depth=4, band=0, single_below=64)


@pytest.mark.parametrize("setting", sorted(OPTIONS))
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_context_options_equal_reference(gpu_api, family, setting):
    """route iv"""
    from ngspeciesid_amd import runtime
    with limit(): api = runtime.new_api(options=OPTIONS[setting])
    try:
        _one_call(api, family, "one call [%s]" % setting, tile_depth=0, band=0)
    finally:
        with limit(): api.close()


def test_stop_when_stable_changes_nothing(gpu_api):
    """route v: identical outputs with and without the switch, one group per call and all in one call - and both equal the reference"""
    gs = pc.family("f_iterations"); ex = pc.expected("f_iterations")
    n = 0
    for sws in (0, 1):
        whole = _call(gpu_api, gs, _prm(gs[0], stop_when_stable=sws), "polish_trace_aln", shuffle_seed=7)
        for g, e, w in zip(gs, ex, whole):
            one = _call(gpu_api, [g], _prm(g, stop_when_stable=sws), "polish_trace_aln")[0]
            assert one[0] == w[0] and [int(u) for u in one[1]] == [int(u) for u in w[1]] and all(np.array_equal(a, b) for a, b in zip(one[2], w[2])), (g.name, sws)
            if not e[3]: continue
            n += 1
            d = pc.differences(e, *one)
            assert not d, "%s [stop_when_stable %d]: %s" % (g.name, sws, "\n".join(d))
    assert n >= 2 * MIN_COMPARED


@pytest.fixture(scope="module")
def threads4_api():
    from ngspeciesid_amd import runtime
    with limit(): api = runtime.new_api(options={"polish_unit_threads": 4})
    yield api
    with limit(): api.close()


def test_unit_threads_stop_when_stable_equals_reference(threads4_api):
    """route vii: family f, stop_when_stable 0 and 1, one call for all groups"""
    gs = pc.family("f_iterations"); ex = pc.expected("f_iterations")
    n = 0
    for sws in (0, 1):
        for g, e, w in zip(gs, ex, _call(threads4_api, gs, _prm(gs[0], stop_when_stable=sws), "polish_trace_aln", shuffle_seed=7)):
            if not e[3]: continue
            n += 1
            d = pc.differences(e, *w)
            assert not d, "%s [unit threads 4, stop_when_stable %d]: %s" % (g.name, sws, "\n".join(d))
    assert n >= 2 * MIN_COMPARED


def test_unit_threads_one_group_per_call_equals_reference(threads4_api):
    """route vii: family d, one group per call"""
    _per_group(threads4_api, "d_strands", "unit threads 4", tile_depth=0, band=0)


def test_subgraph_layers_equal_reference(gpu_api):
    """route vi"""
    gs = pc.family("b_edges"); ex = pc.expected("b_edges", subgraph=True)
    n = 0
    for g, e in zip(gs, ex):
        if not e[3]: continue
        n += 1
        for kw in (dict(tile_depth=0), dict(tile_depth=4, single_below=64)):
            d = pc.differences(e, *_call(gpu_api, [g], _prm(g, subgraph_layers=True, **kw), "polish_trace_aln")[0])
            assert not d, "%s [sub-graph layers, %s]: %s" % (g.name, kw, "\n".join(d))
    assert n >= MIN_COMPARED
    for k, (key, idx) in enumerate(pc.call_keys("b_edges")):
        groups = [gs[x] for x in idx]
        for x, r in zip(idx, _call(gpu_api, groups, _prm(groups[0], subgraph_layers=True), "polish_trace_aln", shuffle_seed=31 + k)):
            if not ex[x][3]: continue
            d = pc.differences(ex[x], *r)
            assert not d, "%s [sub-graph layers, one call]: %s" % (gs[x].name, "\n".join(d))
