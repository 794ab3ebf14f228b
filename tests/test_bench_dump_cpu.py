"""bench.py --dump-outputs: what the timed path returned, written as float32 / float64 .npy files that give the result back exactly, the whole dump under
64 MB with a seeded (repeatable) sample of larger outputs.  The hot path runs on the oracle backend here; bench.py itself needs the GPU
(its usage errors do not)."""
import importlib.util, os, subprocess, sys
import numpy as np
from ngspeciesid_amd import synth, pipeline
from ngspeciesid_amd._capi import ReadSet
from ngspeciesid_amd.hostutil import subset_reads
from ngspeciesid_amd.ptable import select_p_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def _load(d):
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 10 ** 6
    return out


def test_dump_gives_back_the_result_of_the_hot_path(oracle, tmp_path):
    sp = synth.make_species(3, 400, 0.15, seed=2)
    rd = synth.make_reads(sp, 300, mu=17.0, seed=4)
    rs = ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64))
    score, err, keep = oracle.score_reads(rs, 13, 7.0)
    idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
    sub = subset_reads(rs, idx)
    res = pipeline.run_hot_path(oracle, sub, score[idx], acc_rank=np.arange(sub.n, dtype=np.uint32), k=13, w=20, abundance_ratio=0.05, racon_iter=2, p_shared=select_p_table(13, 20))
    assert len(res["centers"]) > 0
    _bench().dump_outputs(str(tmp_path), res)
    d = _load(str(tmp_path))
    for k in ("rep_of", "status", "hpc_err", "counters"):
        assert np.array_equal(d[k], res[k].astype(np.float64)), k
    assert "rep_of_index" not in d and "center_index" not in d                  # small outputs are written whole
    text = lambda nm, i: bytes(d[nm][int(d[nm + "_off"][i]):int(d[nm + "_off"][i + 1])].astype(np.uint8)).decode()
    for i, c in enumerate(res["centers"]):
        assert (d["center_n_reads"][i], d["center_id"][i]) == (c[0], c[1])
        assert text("center_draft", i) == c[2] and text("center_polished", i) == c[3]
        assert list(d["center_groups"][int(d["center_groups_off"][i]):int(d["center_groups_off"][i + 1])]) == c[4]


def test_large_outputs_are_a_seeded_sample_under_64_mb(tmp_path):
    n = 3_000_000
    res = dict(rep_of=np.arange(n, dtype=np.int32)[::-1].copy(), hpc_err=np.linspace(0, 1, n), status=(np.arange(n) % 3).astype(np.uint8),
               counters=np.arange(4, dtype=np.uint64), centers=[(10, i, "A" * 1000, "C" * 999, [i]) for i in range(20000)])
    b = _bench()
    b.dump_outputs(str(tmp_path / "a"), res); b.dump_outputs(str(tmp_path / "b"), res)
    a, a2 = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == sorted(a2) and all(np.array_equal(a[k], a2[k]) for k in a)          # the same sample every time
    ri = a["rep_of_index"].astype(np.int64)
    assert 0 < len(ri) < n and np.all(np.diff(ri) > 0)
    assert np.array_equal(a["rep_of"], res["rep_of"][ri]) and np.array_equal(a["hpc_err"], res["hpc_err"][ri])
    ci = a["center_index"].astype(np.int64)
    assert 0 < len(ci) < 20000 and np.array_equal(a["center_id"], ci) and len(a["center_polished"]) == 999 * len(ci)


def test_check_membership_is_refused_without_full():
    """the membership replay is one of the checks of --full: a plain run that asks for it is a usage error (before anything touches a GPU)"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--check-membership"], timeout=600, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 2 and "--full" in p.stderr and p.stdout == ""
