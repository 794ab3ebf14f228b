"""GPU: the host-side argument checks of the grouped calls, the pair-batch aligners and the alphabet scans come back as return codes, before any kernel of the call runs,
and leave the context usable: the valid form of the same call returns afterwards what it returned before (for poa_consensus and polish: what the oracle returns)."""
import numpy as np
import pytest
from ngspeciesid_amd._capi import NgsidError, ReadSet, poa_params, polish_params

pytestmark = pytest.mark.gpu

N_READS = 6
GRP = np.array([0, 3, 6], dtype=np.uint64)


def _eq(a, b):
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return a == b


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(5)
    tpl = "".join("ACGT"[i] for i in rng.integers(4, size=60))
    reads = []
    for r in range(N_READS):                     # one substitution, and for every second read one deleted base
        a = list(tpl); i = 5 + 8 * r; a[i] = "ACGT"[("ACGT".index(a[i]) + 1 + r % 3) % 4]
        if r % 2: del a[40 + r]
        reads.append("".join(a))
    quals = ["I" * len(s) for s in reads]
    return tpl, reads, ReadSet.from_strings(reads, quals), ReadSet.from_strings([tpl, reads[3]])


def _grouped_calls(api, data):
    """name -> f(grp_off, read_order, centres): the five grouped calls on the reads of `data`"""
    tpl, reads, rs, cen = data
    pp, lp = poa_params(), polish_params(iters=2)
    site_off, site_pos = np.array([0, 1, 2], dtype=np.uint64), np.array([10, 20], dtype=np.uint32)
    return {
        "poa_consensus": lambda g, ro, c: api.poa_consensus(rs, g, pp, read_order=ro),
        "polish": lambda g, ro, c: api.polish(c, rs, g, lp, read_order=ro),
        "polish_trace": lambda g, ro, c: api.polish_trace(c, rs, g, lp, read_order=ro, aln=True),
        "consensus_support": lambda g, ro, c: api.consensus_support(c, rs, g, read_order=ro),
        "phase_genotypes": lambda g, ro, c: api.phase_genotypes(c, rs, g, site_off, site_pos, read_order=ro),
    }


ORDER = np.arange(N_READS, dtype=np.uint32)
GROUP_ERRORS = {
    "read_order entry = number of reads": (GRP, np.array([0, 1, 2, 3, 4, N_READS], dtype=np.uint32), None),
    "offsets one above the number of reads": (np.array([0, 3, N_READS + 1], dtype=np.uint64), None, None),
    "one read under both groups": (GRP, np.array([0, 1, 2, 2, 4, 5], dtype=np.uint32), None),
    "one centre for two groups": (GRP, ORDER, "one"),
}


@pytest.mark.parametrize("name", ["poa_consensus", "polish", "polish_trace", "consensus_support", "phase_genotypes"])
def test_grouped_call_argument_errors(gpu_api, oracle, data, name):
    tpl, reads, rs, cen = data
    call = _grouped_calls(gpu_api, data)[name]
    base = call(GRP, ORDER, cen)
    assert _eq(call(GRP, None, cen), base)
    if name in ("poa_consensus", "polish"):
        assert _eq(_grouped_calls(oracle, data)[name](GRP, ORDER, cen), base), name + ": oracle"
    one = ReadSet.from_strings([tpl])
    for what, (g, ro, c) in GROUP_ERRORS.items():
        if name == "poa_consensus" and what in ("one read under both groups", "one centre for two groups"):
            continue                                   # the draft consensus has no centres and takes a read any number of times
        with pytest.raises(NgsidError) as e:
            call(g, ro, one if c else cen)
        assert e.value.code == -2, (name, what)
        assert _eq(call(GRP, ORDER, cen), base), (name, what, "valid call after the error")


def test_polish_unit_threads_out_of_range(gpu_api, data):
    """polish_unit_threads takes 0 (by the number of pairs) and 1 .. 16: 17 and -1 are refused through the C-ABI (the wrapper's set_option would also remember them
    for the lane contexts), the setting stays what it was and the context polishes as before"""
    import ctypes as C
    tpl, reads, rs, cen = data
    call = _grouped_calls(gpu_api, data)["polish_trace"]
    base = call(GRP, ORDER, cen)
    opt = lambda v: gpu_api.lib.ngsid_ctx_option(gpu_api.ctx, b"polish_unit_threads", C.c_int64(v))
    try:
        assert opt(16) == 0
        for bad in (17, -1):
            assert opt(bad) == -2, bad
            with pytest.raises(NgsidError, match="polish_unit_threads"): gpu_api._err(-2)      # (the message the library left)
            assert _eq(call(GRP, ORDER, cen), base), (bad, "valid call after the error")
    finally:
        assert opt(0) == 0
    assert _eq(call(GRP, ORDER, cen), base)


def test_poa_merge_length_bound(gpu_api, data):
    """Reads whose per-chunk summaries of the merge would run into the sequence bytes in LDS (k_poa.hip MergeLds<64>::max_len = 25 920 bases: 12 bytes per 64 positions
    below LLT<64>::C1 = 4 864) are refused with NGSID_ERR_TOO_LONG before a tile is launched.  match = 2 keeps match x length below 65 536, the explicit band 64 is
    the instance with the smallest bound, node_cap = 22 keeps the graph capacity (1.375 x length nodes, 1.5 x that edges) within the 16-bit indices and
    still holds the edges of two reads; two reads and nothing else, so the upload is the only device work."""
    tpl, reads, rs, cen = data
    rng = np.random.default_rng(11)
    long_ = "".join("ACGT"[i] for i in rng.integers(4, size=25921))      # the plan rounds the longest read up to a multiple of 16: 25 936 > 25 920
    two = ReadSet.from_strings([long_, long_])
    base = gpu_api.poa_consensus(rs, GRP, poa_params())
    with pytest.raises(NgsidError) as e:
        gpu_api.poa_consensus(two, [0, 2], poa_params(match=2, band=64, node_cap=22))
    assert e.value.code == -6
    assert "25920 the merge takes at band width 64" in str(e.value)
    assert _eq(gpu_api.poa_consensus(rs, GRP, poa_params()), base), "valid call after the error"


def _raw_cigar(api, q, t, q_idx, t_idx):
    """ngsid_sg_align_cigar_batch with a column buffer of fixed size -> return code"""
    import ctypes as C
    from ngspeciesid_amd._capi import _p
    qi, ti = np.asarray(q_idx, dtype=np.uint32), np.asarray(t_idx, dtype=np.uint32); n = len(qi)
    open_ = np.full(n, 3, dtype=np.int32); score = np.zeros(n, dtype=np.int32); off = np.zeros(n + 1, dtype=np.uint64); ops = np.zeros(4096, dtype=np.uint8); needed = C.c_uint64(0)
    return api._call("sg_align_cigar_batch", C.byref(q.c), C.byref(t.c), _p(qi), _p(ti), C.c_uint64(n), C.c_int32(2), C.c_int32(-2), _p(open_), C.c_int32(1), _p(score), _p(off), _p(ops),
                     C.c_uint64(len(ops)), C.byref(needed))


@pytest.mark.parametrize("name", ["sg_align_batch", "sg_align_cigar_batch", "ed_align_batch"])
def test_aligner_argument_errors(gpu_api, data, name):
    tpl, reads, rs, cen = data
    q, t = ReadSet.from_strings(reads), cen
    call = {"sg_align_batch": lambda qi, ti: gpu_api.sg_align_batch(q, t, qi, ti, 3),
            "sg_align_cigar_batch": lambda qi, ti: gpu_api.sg_align_cigar_batch(q, t, qi, ti, 3),
            "ed_align_batch": lambda qi, ti: gpu_api.ed_align_batch(q, t, qi, ti)}[name]
    qi, ti = [0, 1, 5], [0, 1, 1]
    base = call(qi, ti)
    assert len(base[0]) == 3
    for bad_q, bad_t in (([0, 1, q.n], ti), (qi, [0, t.n, 1])):
        if name == "sg_align_cigar_batch":
            # the wrapper sizes the column buffer from the lengths of the indexed sequences before it calls the library: an index out of range is numpy's IndexError there.
            with pytest.raises(IndexError):
                call(bad_q, bad_t)
            rc = _raw_cigar(gpu_api, q, t, bad_q, bad_t)      # the library's own check, through the C-ABI
            assert rc == -2, (name, bad_q, bad_t)
        else:
            with pytest.raises(NgsidError) as e:
                call(bad_q, bad_t)
            assert e.value.code == -2, (name, bad_q, bad_t)
        assert _eq(call(qi, ti), base), name
    none = call([], [])
    assert all(len(x) == 0 for x in none), name
    assert _eq(call(qi, ti), base), name


@pytest.mark.parametrize("name", ["demux_locate", "chimera_model"])
def test_alphabet_errors(gpu_api, data, name):
    tpl, reads, rs, cen = data
    if name == "demux_locate":
        call = lambda s: gpu_api.demux_locate(ReadSet.from_strings([s]), [tpl[:12]], window=20)
    else:
        call = lambda s: gpu_api.chimera_model([s], [tpl, reads[3]], [0, 2], [0, 1])
    base = call(reads[0])
    for bad in (reads[0][:-1] + "X", reads[0][:30] + "a" + reads[0][31:]):
        with pytest.raises(NgsidError) as e:
            call(bad)
        assert e.value.code == -3, (name, bad)
        assert _eq(call(reads[0]), base), name
