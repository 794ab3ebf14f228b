"""GPU: the front end - k_score_reads, k_hpc_minimizers in its four layouts, the chunked sparse -> CSR gather, the k > 21 rename pass and k_reads_subset -
against tests/frontend_reference.py (plain Python written from include/ngsid.h, no code shared with oracle/ or the library) on the cases of
tests/frontend_cases.py.  The CPU twin, test_frontend_reference_cpu.py, pins that reference to the reference program's goldens and the oracle to it."""
import ctypes as C
import numpy as np
import pytest
from ngspeciesid_amd._capi import ReadSet, NgsidError
from ngspeciesid_amd.hostutil import subset_reads
import frontend_reference as fr
import frontend_cases as fc

pytestmark = pytest.mark.gpu
SCORE_NAMES, MZ_NAMES = ("score", "err", "keep"), ("mz_off", "codes", "pos", "hpc_len", "hpc_err")
# ngsid_ctx_option settings the results never depend on: the layout of k_hpc_minimizers (1 stored, 2 lean, 3 registers - W <= 32 and one-word codes, else the default -, 4 long)
# and the bases per launch (300: a 750-base read is a chunk of its own, k > 21 carries its second code word from chunk to chunk)
MODES = {"default": None, "stored": dict(minimizers_mode=1), "lean": dict(minimizers_mode=2), "registers": dict(minimizers_mode=3), "long": dict(minimizers_mode=4),
         "chunk300": dict(minimizers_chunk_bases=300)}


@pytest.fixture(scope="module")
def mode_apis(gpu_api):
    """one context per mode for the whole module"""
    from ngspeciesid_amd import runtime
    apis = {}
    try:
        for name, opts in MODES.items():
            apis[name] = gpu_api if opts is None else runtime.new_api(options=opts)
        yield apis
    finally:
        for a in apis.values():
            if a is not gpu_api: a.close()


# ---------------------------------------------------------------------------------------------- score_reads
def test_score_reads_equal_the_reference(gpu_api, oracle):
    """62 calls (6 k x 10 read sets + the two histogram sets, 2 257 reads): score and err bit for bit against the reference AND the oracle, keep everywhere but on the six
    reads built to sit exactly on the threshold (the device log() may differ in the last bit there); host-resident and device-resident input give the same arrays"""
    bad = []
    for i, c in enumerate(fc.score_cases()):
        score, err, keep, phred = fc.score_expected(i)
        rs = fc.read_set(c)
        got = gpu_api.score_reads(rs, c["k"], c["thr"])
        orc = oracle.score_reads(rs, c["k"], c["thr"])
        dev = gpu_api.upload_reads(rs)
        try:
            gdev = gpu_api.score_reads(dev, c["k"], c["thr"])
        finally:
            dev.release()
        on = np.array([t == "on" for t in c["tags"]])
        sel = lambda x: (x[0], x[1], x[2][~on])
        for what, a, b in (("library against the reference", sel(got), (score, err, keep[~on])), ("library against the oracle", sel(got), sel(orc)), ("device-resident against host-resident input", gdev, got)):
            msg = fc.first_difference(c, a, b, SCORE_NAMES, per_read=SCORE_NAMES[:2])
            if msg: bad.append("%s: k = %d, %s" % (what, c["k"], msg))
        for r, t in enumerate(c["tags"]):
            if t in ("above", "below") and got[2][r] != (t == "above"): bad.append("%s: keep of the read just %s the threshold is %d" % (c["name"], t, got[2][r]))
    print("%d score calls, %d reads" % (len(fc.score_cases()), sum(len(c["seqs"]) for c in fc.score_cases())))
    assert not bad, "\n".join(bad[:20])


def test_score_reads_k_above_64_is_an_argument_error(gpu_api):
    rs = ReadSet.from_strings(["ACGT" * 40], ["5" * 160])
    with pytest.raises(NgsidError) as e:
        gpu_api.score_reads(rs, 65, 7.0)
    assert e.value.code == -2                                      # NGSID_ERR_ARG: the quality ring holds 128 characters
    assert gpu_api.score_reads(rs, 64, 7.0)[2][0] == 1


# ---------------------------------------------------------------------------------------------- hpc_minimizers
@pytest.mark.parametrize("mode", list(MODES))
def test_hpc_minimizers_equal_the_reference(mode_apis, mode):
    """per mode 92 calls (22 (k, w) pairs x {with qualities, without, alphabet error}, the alphabet error in a read without a k-mer for the 20 pairs with k > 1, and the six
    one-minimizer calls of k > 21): mz_off, codes (k > 21: ranks), pos,
    hpc_len and hpc_err (NaN without qualities) equal the reference.  `registers` with W = 33 ((16, 48)) or k > 21 falls back to the default layout and still agrees."""
    api = mode_apis[mode]
    bad, calls = [], 0
    for i, c in enumerate(fc.minimizer_cases()):
        exp = fc.minimizer_expected(i)
        calls += 1
        where = "mode %s, k = %d, w = %d" % (mode, c["k"], c["w"])
        if c["bad"]:
            # a base outside ACGTN in reads 3 and 7: one wave per read, both raise the flag and either may be the one the message names
            with pytest.raises(NgsidError) as e:
                api.hpc_minimizers(fc.read_set(c), c["k"], c["w"])
            if e.value.code != -3 or not any(("read %d:" % r) in str(e.value) for r in c["bad"]): bad.append("%s: %s: %s" % (where, c["name"], e.value))
            continue
        got = api.hpc_minimizers(fc.read_set(c), c["k"], c["w"])
        msg = fc.first_difference(c, got, exp, MZ_NAMES, per_read=MZ_NAMES[3:])
        if msg:
            nm = msg.split(": ")[1].split("[")[0]
            if nm in ("codes", "pos"):                             # name the read the entry belongs to
                x = int(msg.split("[")[1].split("]")[0]); r = int(np.searchsorted(exp[0], x, side="right")) - 1
                msg += " - minimizer %d of %s" % (x - int(exp[0][r]), fc.describe_read(c, r))
            bad.append("%s: %s" % (where, msg))
    print("mode %s: %d calls" % (mode, calls))
    assert not bad, "\n".join(bad[:20])


def test_cluster_greedy_refuses_a_foreign_base_in_a_read_without_a_kmer(gpu_api, oracle):
    """the clustering sketches its reads with the same kernel: an X in a read of HPC length < k (which would only be skipped as NGSID_ST_SHORT) is NGSID_ERR_ALPHABET too,
    from the library and from the oracle"""
    from ngspeciesid_amd._capi import cluster_params
    from ngspeciesid_amd.ptable import select_p_table
    rng = np.random.default_rng(9)
    seqs = [fc.no_hp(rng, 80, "ACGT") for _ in range(5)] + ["ACGXACG"] + [fc.no_hp(rng, 80, "ACGT") for _ in range(3)]
    rs = ReadSet.from_strings(seqs, [fc.rand_qual(rng, len(s)) for s in seqs])
    for api in (gpu_api, oracle):
        with pytest.raises(NgsidError) as e:
            api.cluster_greedy(rs, cluster_params(k=13, w=20, p_shared=select_p_table(13, 20)))
        assert e.value.code == -3 and "read 5:" in str(e.value)


# ---------------------------------------------------------------------------------------------- reads_subset
def _hip():
    """the HIP runtime the library has loaded already"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in this process")


def _from_device(ptr, count, dtype):
    out = np.zeros(count, dtype=dtype)
    if count:
        rc = _hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(int(ptr)), C.c_size_t(out.nbytes), C.c_int(2))       # 2 = hipMemcpyDeviceToHost
        assert rc == 0, "hipMemcpy: %d" % rc
    return out


def _subset_source(with_qual):
    """300 reads of 0 .. 200 bases; empty reads, lower-case bases and X in a few"""
    rng = np.random.default_rng(31)
    seqs = [fc.rand_seq(rng, int(n), "ACGTN") for n in rng.integers(1, 201, 300)]
    for r in (0, 17, 150, 299): seqs[r] = ""
    for r in (3, 40, 41, 298): seqs[r] = seqs[r][:1].lower() + seqs[r][1:-1] + "x" * (len(seqs[r]) > 1)
    for r in (5, 41, 200): seqs[r] = seqs[r] + "X"
    return seqs, ([fc.rand_qual(rng, len(s)) for s in seqs] if with_qual else None)


@pytest.mark.parametrize("with_qual", [True, False], ids=["qual", "noqual"])
def test_reads_subset_equals_the_host_gather(gpu_api, with_qual):
    """k_reads_subset (four reads per workgroup) on seven index lists: the device result, copied back, equals hostutil.subset_reads byte for byte, `foreign` counts the
    bytes outside ACGTN, and score_reads on the device subset equals score_reads on the host subset"""
    seqs, quals = _subset_source(with_qual)
    host = ReadSet.from_strings(seqs, quals)
    rng = np.random.default_rng(32)
    lists = dict(identity=np.arange(300), reversal=np.arange(300)[::-1], repeats=rng.integers(0, 300, 500), one=[41], four=[298, 0, 3, 3], five=[5, 299, 200, 40, 17], empty=[])
    dev = gpu_api.upload_reads(host)
    made = []
    try:
        for name, idx in lists.items():
            idx = np.asarray(idx, dtype=np.int64)
            sub, foreign = gpu_api.reads_subset(dev, idx); made.append(sub)
            want = subset_reads(host, idx)
            total = int(want.off[-1])
            assert sub.n == len(idx) == want.n, name
            assert np.array_equal(_from_device(sub.off, len(idx) + 1, np.uint64), want.off), name
            assert np.array_equal(_from_device(sub.seq, total, np.uint8), want.seq[:total]), name
            if with_qual: assert np.array_equal(_from_device(sub.qual, total, np.uint8), want.qual[:total]), name
            else: assert sub.qual is None, name
            assert foreign == sum(ch not in "ACGTN" for i in idx for ch in seqs[i]), name
            if with_qual:
                for a, b in zip(gpu_api.score_reads(sub, 13, 7.0), gpu_api.score_reads(want, 13, 7.0)):
                    assert np.array_equal(a, b), name
        with pytest.raises(NgsidError) as e:
            gpu_api.reads_subset(dev, [0, 300])
        assert e.value.code == -2                                  # NGSID_ERR_ARG: index out of range
    finally:
        for s in made: s.release()
        dev.release()
