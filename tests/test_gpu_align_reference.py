"""GPU: the semi-global affine aligners (k_sg_align, k_sg_align16, k_sg_align16p and their shared traceback walk) against the plain reference of their
contract (align_reference.py) on the edge families of align_cases.py - score, n_cols, n_match, region and the alignment columns, exactly (integers: no
tolerance) - under the context options that choose the kernel and the route.  include/ngsid.h: results never depend on them.

A mismatch names the family's call, the pair and its tag, (n, m), open, the scheme, the reference value and the setting; for a class-routed call also
the length class of the pair and its residue bin (n - 1) mod R.  Every library call runs under a time limit of its own: a hang ends the process
(faulthandler) instead of the next step being started on the same device.
"""
import contextlib, ctypes as C, faulthandler, sys
import numpy as np
import pytest
from ngspeciesid_amd._capi import NgsidError, ReadSet, _p, polish_params
import align_cases as ac
import align_reference as ref

pytestmark = pytest.mark.gpu
STEP_LIMIT = 120      # seconds per library call (they take milliseconds)
SETTINGS = {"default": {}, "align32": {"align32": 1}}
F_SETTINGS = {"default": {}, "skew0": {"align_skew": 0}, "paired0": {"align_paired": 0}, "noclass": {"align_noclass": 1}, "align32": {"align32": 1}}
NAMES = ("score", "n_cols", "n_match", "region")
_sets = {}


@contextlib.contextmanager
def limit(seconds=STEP_LIMIT):
    faulthandler.dump_traceback_later(seconds, exit=True, file=sys.stderr)
    try: yield
    finally: faulthandler.cancel_dump_traceback_later()


@contextlib.contextmanager
def context(options):
    from ngspeciesid_amd import runtime
    api = runtime.new_api(options=options)
    try: yield api
    finally: api.close()


def read_sets(case):
    if case.name not in _sets: _sets[case.name] = (ReadSet.from_strings(list(case.queries)), ReadSet.from_strings(list(case.targets)))
    return _sets[case.name]


def run(api, case, upto=None):
    Q, T = read_sets(case); s = slice(0, upto)
    with limit():
        return api.sg_align_batch(Q, T, case.q_idx[s], case.t_idx[s], case.open[s], ext=case.ext, match=case.match, mismatch=case.mismatch, k=case.k,
                                  match_id=None if case.mid_absent else case.match_id[s])


def run_cigar(api, case, at=None):
    Q, T = read_sets(case); at = slice(None) if at is None else at
    with limit():
        return api.sg_align_cigar_batch(Q, T, case.q_idx[at], case.t_idx[at], case.open[at], ext=case.ext, match=case.match, mismatch=case.mismatch)


def where(case, p, routed=False):
    q, t = case.queries[case.q_idx[p]], case.targets[case.t_idx[p]]; n = len(q)
    tag = case.tags[p] if isinstance(case.tags[p], str) else case.tags[p]["what"]
    s = "family %s, %s, pair %d (%s), n %d, m %d, open %d, %d/%d/ext %d, k %d, match_id %d" % (case.family, case.name, p, tag, n, len(t), case.open[p], case.match, case.mismatch, case.ext, case.k, case.match_id[p])
    if routed:
        c = ac.class_of(n); R = ac.CLASSES[c][2]
        s += ", class %d" % c + (" (int32: m > %d)" % ac.ALIGN16_MAXLEN if len(t) > ac.ALIGN16_MAXLEN else ", residue %d of R = %d" % ((n - 1) % R, R) if R and n else "")
    return s


def check(case, got, exp, setting, at=None, what="reference", routed=False, names=NAMES):
    """got / exp: arrays over the pairs of the call; at: the pairs compared (default: those the case checks against the reference)"""
    at = np.nonzero(case.ref)[0] if at is None else at
    for nm, a, b in zip(names, got, exp):
        bad = at[a[at] != b[at]]
        if len(bad):
            p = int(bad[0])
            pytest.fail("%s differs from the %s for %d of %d pairs [%s]; first: %s: got %d, %s %d" % (nm, what, len(bad), len(at), setting, where(case, p, routed), a[p], what, b[p]))


def check_columns(case, cols, exp_cols, setting, at):
    for x, p in enumerate(at):
        if cols[x] != exp_cols[p]:
            d = next((y for y, (a, b) in enumerate(zip(cols[x], exp_cols[p])) if a != b), min(len(cols[x]), len(exp_cols[p])))
            pytest.fail("columns differ from the reference [%s]; %s; first difference at column %d of %d / %d\n  got       ...%s\n  reference ...%s"
                        % (setting, where(case, int(p)), d, len(cols[x]), len(exp_cols[p]), cols[x][max(0, d - 20):d + 40], exp_cols[p][max(0, d - 20):d + 40]))


@pytest.mark.parametrize("family,setting", [(f, s) for f in "abcdeg" for s in SETTINGS])
def test_family_equals_reference(gpu_api, family, setting):
    """every output of sg_align_batch and the columns (and score) of sg_align_cigar_batch, the int16 route and the int32 one"""
    with context(SETTINGS[setting]) as api:
        for case in ac.cases(family):
            r = ref.case_results(case)
            check(case, run(api, case), r[:4], setting)
            at = np.nonzero(case.ref)[0]
            sc, cols = run_cigar(api, case)
            check(case, (sc,), (r[0],), setting + ", cigar call", names=("score",))
            check_columns(case, cols, r[4], setting + ", cigar call", at)


def test_window_above_64_is_an_argument_error(gpu_api):
    case = ac.cases("d")[0]; Q, T = read_sets(case)
    with context({}) as api:
        for k in (65, 1000):
            with pytest.raises(NgsidError) as e, limit():
                api.sg_align_batch(Q, T, case.q_idx, case.t_idx, case.open, k=k)
            assert e.value.code == -2, e.value
        check(case, run(api, case), ref.case_results(case)[:4], "after the refused calls")


def test_partitioned_batch_equals_reference_oracle_and_itself(gpu_api, oracle):
    """family f: 4 096 + 7 pairs in one call - the length classes on side streams, the paired kernel in its skewed and plain frame, the one-pair kernel per class, one launch
    without classes, and int32: the edge pairs against the reference, every pair against the oracle, all settings equal; and the first 4 095 pairs (one launch) the same per pair"""
    (case,) = ac.cases("f")
    Q, T = read_sets(case); r = ref.case_results(case)
    exp = oracle.sg_align_batch(Q, T, case.q_idx, case.t_idx, case.open, ext=case.ext, match=case.match, mismatch=case.mismatch, k=case.k, match_id=case.match_id)
    every = np.arange(len(case.q_idx)); first = None
    for setting, opts in F_SETTINGS.items():
        with context(opts) as api:
            got = run(api, case)
            check(case, got, r[:4], setting, routed=True)
            check(case, got, exp, setting, at=every, what="oracle", routed=True)
            if first is None: first = got
            check(case, got, first, setting, at=every, what="default setting", routed=True)
            cut = run(api, case, upto=ac.PARTITION_MIN_PAIRS - 1)
            check(case, cut, [a[:len(cut[0])] for a in first], setting + ", the first 4 095 pairs alone", at=every[:len(cut[0])], what="whole batch", routed=True)
    at = np.nonzero(case.ref)[0]
    with context({}) as api:
        sc, cols = run_cigar(api, case, at)
        assert np.array_equal(sc, r[0][at])
        check_columns(case, cols, r[4], "default, cigar call", at)


def _c_call(api, case, want, with_match_id):
    """the C entry point with NULL for the outputs not in `want`"""
    Q, T = read_sets(case); n = len(case.q_idx)
    out = {k: np.full(n, -7, dtype=np.int32) for k in NAMES}
    f = api.lib.ngsid_sg_align_batch; f.restype = C.c_int32
    with limit():
        rc = f(api.ctx, C.byref(Q.c), C.byref(T.c), _p(case.q_idx), _p(case.t_idx), C.c_uint64(n), C.c_int32(case.match), C.c_int32(case.mismatch), _p(case.open), C.c_int32(case.ext),
               C.c_int32(case.k), _p(case.match_id) if with_match_id else None, *[_p(out[k]) if k in want else None for k in NAMES])
    assert rc == 0, (case.name, want, rc)
    return out


@pytest.mark.parametrize("want", [("score",), ("n_cols",), ("n_match",), ("region",), ("score", "region"), ()], ids=lambda w: "+".join(w) or "none")
def test_optional_outputs(gpu_api, want):
    """'any output may be NULL': each output requested alone equals the reference and the others stay untouched; match_id NULL means k"""
    with context({}) as api:
        for case in (ac.cases("g")[0], ac.cases("d")[5], ac.cases("c")[1]):
            r = dict(zip(NAMES, ref.case_results(case)[:4]))
            part = _c_call(api, case, want, with_match_id=not case.mid_absent)
            for k in NAMES:
                if k in want: check(case, (part[k],), (r[k],), "only %s requested" % ("+".join(want)), names=(k,))
                else: assert (part[k] == -7).all(), (case.name, k, "written though not requested")
            if (case.match_id == case.k).all():
                both = _c_call(api, case, NAMES, with_match_id=True)
                check(case, [both[k] for k in NAMES], [r[k] for k in NAMES], "match_id given and equal to k")


def test_same_context_again_after_a_larger_call(gpu_api):
    """scratch only grows and the class launches of a partitioned batch run on side streams: small calls, then the partitioned batch (more pairs, a 4 001-base target), then
    the small calls again on the same context - identical to the first time and equal to the reference"""
    small = [ac.cases("g")[0], [c for c in ac.cases("a") if c.name == "a_L769"][0], [c for c in ac.cases("b") if c.name == "b_L2304"][0]]
    (big,) = ac.cases("f")
    assert len(big.q_idx) > max(len(c.q_idx) for c in small) and max(map(len, big.targets)) > max(len(t) for c in small for t in c.targets)
    with context({}) as api:
        first = [run(api, c) for c in small]
        check(big, run(api, big), ref.case_results(big)[:4], "between the small calls", routed=True)
        for c, one in zip(small, first):
            two = run(api, c)
            check(c, two, one, "second run", what="first run")
            check(c, two, ref.case_results(c)[:4], "second run")
            sc, cols = run_cigar(api, c)
            check_columns(c, cols, ref.case_results(c)[4], "second run, cigar call", np.nonzero(c.ref)[0])


# ---- family s: the spans of the polisher's affine read -> backbone alignment (aln_mode 0)
_span_cache = {}


def _expected_record(group, x):
    """{strand, q_begin, q_end, t_begin, t_end, -1} of include/ngsid.h from the reference's span of the oriented read against the backbone"""
    key = (group.name, x)
    if key not in _span_cache:
        read = group.reads[x]; s = group.strand[x]
        r = ref.align_pair(ac.revcomp(read) if s else read, group.backbone, ac.S_SCORES["aln_match"], ac.S_SCORES["aln_mismatch"], ac.S_SCORES["aln_open"], ac.S_SCORES["aln_ext"])
        qf, ql, tf, tl = r.span
        assert qf >= 0
        _span_cache[key] = [s, len(read) - 1 - ql if s else qf, len(read) - qf if s else ql + 1, tf, tl + 1, -1]
    return _span_cache[key]


def _polish_records(api, groups):
    bb = ReadSet.from_strings([g.backbone for g in groups]); rs = ReadSet.from_strings([r for g in groups for r in g.reads])
    off = np.concatenate(([0], np.cumsum([len(g.reads) for g in groups])))
    prm = polish_params(iters=1, window=500, k=13, w=20, tile_depth=6, band=0, trim=2, aln_mode=0, stop_when_stable=0, **ac.S_SCORES)
    with limit():
        _, _, rec = api.polish_trace(bb, rs, off, prm, aln=True)
    return np.asarray(rec)[0], off


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_polisher_spans_equal_reference(gpu_api, setting):
    """backbones of 499 ... 1 050 bases (one, two and three polishing windows: the walk's window-boundary branch runs), plus and minus reads: the PAF record of every read"""
    groups = ac.family_s()
    with context(SETTINGS[setting]) as api:
        rec, off = _polish_records(api, groups)
    for g, grp in enumerate(groups):
        for x in range(len(grp.reads)):
            exp = _expected_record(grp, x); got = rec[off[g] + x].tolist()
            assert got == exp, "family s, %s (backbone %d), read %d (n %d, strand %d) [%s]: got %s, reference %s" % (grp.name, len(grp.backbone), x, len(grp.reads[x]), grp.strand[x], setting, got, exp)


def test_polisher_spans_of_a_partitioned_call(gpu_api):
    """more than 4 096 reads in one polishing call (the aligner partitions them: the paired kernel writes the spans) with align_paired 1 and 0: identical, and 200 reads
    equal the reference"""
    many, checked = ac.family_s_many()
    recs = {}
    for paired in (1, 0):
        with context({"align_paired": paired}) as api:
            recs[paired], _ = _polish_records(api, [many])
    for x in checked:
        exp = _expected_record(many, x); got = recs[1][x].tolist()
        c = ac.class_of(len(many.reads[x])); R = ac.CLASSES[c][2]
        assert got == exp, "family s, s_many read %d (n %d, strand %d, class %d, residue %d) [align_paired 1]: got %s, reference %s" % (x, len(many.reads[x]), many.strand[x], c, (len(many.reads[x]) - 1) % R, got, exp)
    bad = np.nonzero((recs[1] != recs[0]).any(axis=1))[0]
    assert len(bad) == 0, "align_paired 1 and 0 differ for %d reads; first: read %d (n %d): %s against %s" % (len(bad), bad[0], len(many.reads[bad[0]]), recs[1][bad[0]].tolist(), recs[0][bad[0]].tolist())
