"""GPU: the edit-distance polisher aligner (k_ed_align) against the plain reference of its contract (ed_reference.py) on the edge families of
ed_cases.py - distance, span and window break points, exactly (integers: no tolerance) - under the scheduling options that select its
instances and launches.  include/ngsid.h: results never depend on them.

A mismatch names the family's call, the pair, (n, m), the reference distance and the pair's lane in its 64-pair bundle of the call order.
"""
import ctypes as C
import numpy as np
import pytest
from ngspeciesid_amd._capi import ReadSet, _p
import ed_cases
import ed_reference as ref

SETTINGS = {"default": {}, "win_all0": {"ed_win_all": 0}, "win6_0": {"ed_win6": 0}, "noclass": {"align_noclass": 1}}
for _b in (0, 12, 40, 100, 150, 151, 400): SETTINGS["band%d" % _b] = {"ed_band": _b}
BANDS = ["band0", "band12", "band40", "band100", "band150", "band151", "band400"]
MATRIX = {"a": ["default", "band0", "band12", "band40", "band150", "band400"],
          "b": ["default"] + BANDS,
          "c": ["default"] + BANDS,
          "d": ["default", "band0", "band12"],
          "e": ["default", "band0", "band12"],
          "f": ["default", "band0", "band150", "band151", "band400"],
          "g": ["default", "win_all0", "win6_0", "noclass", "band100", "band150", "band151"]}
_sets = {}


def read_sets(case):
    if case.name not in _sets: _sets[case.name] = (ReadSet.from_strings(case.queries), ReadSet.from_strings(case.targets))
    return _sets[case.name]


def check(case, got, exp, what=("distance", "span", "bp"), note=""):
    for nm, a, b in zip(what, got, exp):
        assert a.shape == b.shape, (case.name, nm, a.shape, b.shape)
        bad = np.nonzero((a != b).reshape(len(case.q_idx), -1).any(axis=1))[0]
        if len(bad):
            p = int(bad[0]); n = len(case.queries[case.q_idx[p]]); m = len(case.targets[case.t_idx[p]])
            w = np.nonzero((a[p] != b[p]).reshape(-1, 4).any(axis=1))[0][:3] if nm == "bp" else None
            pytest.fail("%s%s: %s differs for %d of %d pairs; first: pair %d (%s), n %d, m %d, reference distance %d, lane %d of bundle %d (window %d, bp_windows %d)%s\n  got      %s\n  expected %s"
                        % (case.name, note, nm, len(bad), len(case.q_idx), p, case.tags[p], n, m, ref.case_results(case)[0][p], p % 64, p // 64, case.window, case.bp_windows,
                           "" if w is None else ", windows %s" % w.tolist(), (a[p][w] if w is not None else a[p]).tolist(), (b[p][w] if w is not None else b[p]).tolist()))


def run(api, case):
    Q, T = read_sets(case)
    return api.ed_align_batch(Q, T, case.q_idx, case.t_idx, window=case.window, bp_windows=case.bp_windows)


@pytest.mark.gpu
@pytest.mark.parametrize("family,setting", [(f, s) for f in sorted(MATRIX) for s in MATRIX[f]])
def test_family_equals_reference(gpu_api, family, setting):
    from ngspeciesid_amd import runtime
    api = runtime.new_api(options=SETTINGS[setting])
    try:
        for case in ed_cases.cases(family):
            check(case, run(api, case), ref.case_results(case), note=" [%s]" % setting)
    finally:
        api.close()


def _c_call(api, case, want):
    """the C entry point with NULL for the outputs not in `want`"""
    Q, T = read_sets(case); n = len(case.q_idx)
    out = {"distance": np.full(n, -7, dtype=np.int32), "span": np.full((n, 4), -7, dtype=np.int32), "bp": np.full((n, case.bp_windows, 4), -7, dtype=np.int32)}
    f = api.lib.ngsid_ed_align_batch; f.restype = C.c_int32
    rc = f(api.ctx, C.byref(Q.c), C.byref(T.c), _p(case.q_idx), _p(case.t_idx), C.c_uint64(n), C.c_int32(case.window), C.c_int32(case.bp_windows),
           *[_p(out[k]) if k in want else None for k in ("distance", "span", "bp")])
    assert rc == 0, (case.name, want, rc)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("want", [("distance",), ("span",), ("bp",), ("distance", "span"), ("distance", "bp"), ("span", "bp")], ids="+".join)
def test_optional_outputs(gpu_api, want):
    """'any may be NULL': each output requested alone and in pairs equals the call with all three (and with it the reference)"""
    from ngspeciesid_amd import runtime
    api = runtime.new_api(options={})
    try:
        for case in (ed_cases.cases("c")[2], ed_cases.cases("e")[9], ed_cases.cases("d")[0]):
            full = _c_call(api, case, ("distance", "span", "bp"))
            check(case, [full[k] for k in ("distance", "span", "bp")], ref.case_results(case), note=" [C entry point, all outputs]")
            part = _c_call(api, case, want)
            check(case, [part[k] for k in want], [full[k] for k in want], what=want, note=" [only %s requested]" % "+".join(want))
            for k in part:
                if k not in want: assert (part[k] == -7).all(), (case.name, k, "written though not requested")
    finally:
        api.close()


@pytest.mark.gpu
def test_same_context_again_after_a_longer_target(gpu_api):
    """the traceback scratch only grows and its column stride follows the longest target of the CALL: family c (targets up to 1 500 bases), then a call
    with a 3 200-base target, then family c again on the same context - identical, and equal to the reference"""
    from ngspeciesid_amd import runtime
    api = runtime.new_api(options={})
    try:
        cs = ed_cases.cases("c")
        first = [run(api, case) for case in cs]
        longer = ed_cases.cases("e")[10]
        assert max(len(t) for t in longer.targets) > 2 * max(len(t) for c in cs for t in c.targets)
        check(longer, run(api, longer), ref.case_results(longer))
        for case, one in zip(cs, first):
            two = run(api, case)
            check(case, two, one, note=" [second run vs first]")
            check(case, two, ref.case_results(case), note=" [second run]")
    finally:
        api.close()

