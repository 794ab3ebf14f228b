"""What the five consumers of the store pass must return for a case of rec_cases.py, from their references (support_, cigar_, phase_, hp_, errprof_reference.py) with the
columns and strands of a chosen source - by default tests/columns_reference.py, which involves no oracle.  Computed once per (case, source), shared, read-only."""
import numpy as np
from ngspeciesid_amd._capi import ReadSet
import columns_reference
from support_reference import support_reference
from cigar_reference import cigar_reference
from phase_reference import genotypes_reference
from hp_reference import hp_reference
from errprof_reference import errprof_reference

_sets = {}
_exp = {}
CALLS = ("support", "cigar", "cigar_m", "geno", "hp", "errprof")


def read_sets(case):
    """(centres, reads with qualities) as ReadSets"""
    if case.name not in _sets: _sets[case.name] = (ReadSet.from_strings(case.centres), ReadSet.from_strings(case.reads, case.quals))
    return _sets[case.name]


def _freeze(t):
    for a in t:
        if isinstance(a, np.ndarray): a.setflags(write=False)
    return t


def expected(case, what, oracle=None, source=columns_reference):
    """the tuple that Api.consensus_support / read_cigars (what = "cigar", with merge_m "cigar_m") / phase_genotypes / hp_runs / error_profile returns"""
    key = (case.name, what, None if source is None else source.__name__)
    if key not in _exp:
        _, rs = read_sets(case)
        a = (oracle, case.centres, rs, case.grp_off)
        kw = dict(read_order=case.read_order, k=case.k, w=case.w, clip=case.clip, source=source)
        if what == "support": r = support_reference(*a, **kw)
        elif what == "cigar": r = cigar_reference(*a, **kw)
        elif what == "cigar_m": r = cigar_reference(*a, merge_m=True, **kw)
        elif what == "geno": r = genotypes_reference(*a, case.site_off, case.site_pos, **kw)
        elif what == "hp": r = hp_reference(*a, case.run_off, case.run_start, **kw)
        else: r = errprof_reference(*a, **kw)
        _exp[key] = _freeze(tuple(r))
    return _exp[key]


def listed_columns(case):
    """per listed read (strand, oriented read, column list or None without a strand) from columns_reference"""
    _, rs = read_sets(case)
    st = columns_reference.strands(case.centres, rs, case.grp_off, case.read_order, case.k, case.w)
    out = []
    for g in range(len(case.centres)):
        for x in range(int(case.grp_off[g]), int(case.grp_off[g + 1])):
            if st[x] < 0: out.append((-1, None, None)); continue
            r = columns_reference.oriented(case.reads[int(case.read_order[x])], int(st[x]))
            out.append((int(st[x]), r, columns_reference.ed_ops(r, case.centres[g])))
    return out


def group_of(case, x):
    return int(np.searchsorted(np.asarray(case.grp_off), x, side="right")) - 1
