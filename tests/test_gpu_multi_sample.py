"""GPU: multi-sample batch mode (include/ngsid_batch.h, pipeline.run_hot_path_samples): every sample of a batch gets exactly the result it gets when it is run alone.

The last tests run the `--fastq_dir` mode of the command line against one run per file."""
import ctypes as C
import numpy as np
import pytest
from ngspeciesid_amd import runtime, synth, pipeline, _capi
from ngspeciesid_amd._capi import ReadSet, cluster_params, polish_params, NgsidError
from ngspeciesid_amd.hostutil import subset_reads
from ngspeciesid_amd.ptable import select_p_table

pytestmark = pytest.mark.gpu


def _concat(sets):
    seq = np.concatenate([s.seq for s in sets]) if sets else np.zeros(0, np.uint8)
    qual = np.concatenate([s.qual for s in sets]) if sets else np.zeros(0, np.uint8)
    lens = np.concatenate([np.diff(s.off.astype(np.int64)) for s in sets]) if sets else np.zeros(0, np.int64)
    off = np.zeros(len(lens) + 1, dtype=np.uint64); off[1:] = np.cumsum(lens)
    seg = np.zeros(len(sets) + 1, dtype=np.uint64); seg[1:] = np.cumsum([s.n for s in sets])
    return ReadSet(seq, qual, off), seg


def _sample(api, species, n, seed, k=13, mu=15.0, abundance=None, rc_fraction=0.2):
    """one demultiplexed sample in score order -> (ReadSet, score)"""
    rd = synth.make_reads(species, n, mu=mu, seed=seed, abundance=abundance, rc_fraction=rc_fraction)
    rs0 = ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64))
    score, err, keep = api.score_reads(rs0, k, 7.0)
    idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
    return subset_reads(rs0, idx), score[idx]


def _fixed(strings):
    return ReadSet.from_strings(strings, ["5" * len(s) for s in strings])


def _batch(api, k=13):
    """seven samples of unequal size from the same five amplicons + an empty segment, a one-read segment, a segment of reads shorter than k and a byte-identical copy of a sample
    -> (sets, index of the copied sample, index of its copy)"""
    sp = synth.make_species(5, 500, 0.12, seed=41)
    sizes = [50, 3000, 400, 1200, 800, 150, 2000]
    s = [_sample(api, sp, n, 100 + i, k=k, mu=14.0 + (i % 3))[0] for i, n in enumerate(sizes)]
    empty = ReadSet(np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    single = subset_reads(s[3], np.arange(7, 8))
    short = _fixed(["ACGTAC", "ACGTACGT", "TTGACA", "ACGTAC"])
    sets = [s[0], s[1], s[2], empty, s[3], single, s[4], short, s[5], s[6], subset_reads(s[2], np.arange(s[2].n))]
    return sets, 2, 10


def _alone(api, sets, prm, acc):
    """ngsid_cluster_greedy per segment, rep_of mapped to indices of the whole set"""
    rep, herr, st, cnt = [], [], [], []
    base = 0
    for x in sets:
        if x.n:
            r, h, t, c = api.cluster_greedy(x, prm, acc_rank=acc[base:base + x.n])
        else:
            r, h, t, c = np.zeros(0, np.int32), np.zeros(0), np.zeros(0, np.uint8), np.zeros(4, np.uint64)
        rep.append(r.astype(np.int64) + base); herr.append(h); st.append(t); cnt.append(c); base += x.n
    return np.concatenate(rep), np.concatenate(herr), np.concatenate(st), np.stack(cnt)


def _same(got, want, what):
    rep, herr, st, cnt = got
    assert np.array_equal(rep.astype(np.int64), want[0]), what + ": rep_of"
    assert np.array_equal(st, want[2]), what + ": status"
    assert np.array_equal(herr.view(np.uint64), want[1].view(np.uint64)), what + ": hpc_err bit for bit"
    assert np.array_equal(cnt, want[3]), what + ": counters per segment"


@pytest.mark.parametrize("k,w", [(13, 20), (15, 50), (25, 30)])
def test_segmented_equals_every_segment_alone(oracle, k, w):
    """(13, 20) also under a fixed small block, a cut of restarting blocks and the end-to-end item order; (25, 30) is the dense-rank code path"""
    with runtime.new_api() as api:
        sets, orig, copy = _batch(api, k=13)
        rs, seg = _concat(sets)
        assert rs.n > 7000 and len(seg) == 12
        prm = cluster_params(k=k, w=w, p_shared=select_p_table(k, w))
        acc = np.arange(rs.n, dtype=np.uint32)
        want = _alone(api, sets, prm, acc)
        _same(_alone(oracle, sets, prm, acc), want, "oracle per segment vs library per segment")
        variants = [dict()] if k != 13 else [dict(), dict(cluster_block=4096), dict(cluster_block=4096, cluster_trunc=500), dict(cluster_seg_order=1), dict(cluster_seg_order=1, cluster_block=4096)]
        for opt in variants:
            for name, dflt in (("cluster_block", 0), ("cluster_trunc", 32768), ("cluster_seg_order", 0)):
                assert api.lib.ngsid_ctx_option(api.ctx, name.encode(), C.c_int64(opt.get(name, dflt))) == 0
            got = api.cluster_greedy_segmented(rs, prm, seg, acc_rank=acc)
            _same(got, want, "segmented %s" % opt)
            # isolation: no read carries a representative outside its segment; the copied sample gets the original's result, shifted
            sg = np.searchsorted(seg.astype(np.int64), np.arange(rs.n), side="right") - 1
            assert np.array_equal(sg[got[0]], sg)
            a0, a1, b0, b1 = int(seg[orig]), int(seg[orig + 1]), int(seg[copy]), int(seg[copy + 1])
            assert np.array_equal(got[0][a0:a1] - a0, got[0][b0:b1] - b0) and np.array_equal(got[2][a0:a1], got[2][b0:b1]) and np.array_equal(got[3][orig], got[3][copy])
        assert want[3][3].sum() == 0 and want[3][7].sum() == 0 and (want[2][int(seg[7]):int(seg[8])] == _capi.ST_SHORT).all()
        assert want[3][5].tolist() == [0, 0, 0, 1]


def test_minimizer_cache_is_not_poisoned():
    """the tagged codes of a segmented call must not serve the polisher's strand detection: ngsid_polish on the same reads returns the bytes of a fresh context"""
    sp = synth.make_species(3, 500, 0.12, seed=43)
    with runtime.new_api() as api, runtime.new_api() as fresh:
        a, _ = _sample(api, sp, 900, 7); b, _ = _sample(api, sp, 700, 8)
        rs, seg = _concat([a, b])
        assert rs.n >= 1024                                                     # the size from which the cache is keyed at all
        prm = cluster_params(k=13, w=20, p_shared=select_p_table(13, 20))
        dev = api.upload_reads(rs); dev2 = fresh.upload_reads(rs)
        try:
            plain = api.cluster_greedy(dev, prm)                                # a plain call first: it leaves the cache VALID for these reads, the segmented call must take that back
            rep, _, _, _ = api.cluster_greedy_segmented(dev, prm, seg)
            assert not np.array_equal(plain[0], rep)                            # (the same amplicons in both samples: clustered together they share representatives)
            reps, order, grp_off, counts = pipeline.clusters_from_rep(rep)
            big = [g for g in np.argsort(-counts)[:4] if counts[g] >= 20]
            lists = [order[int(grp_off[g]):int(grp_off[g + 1])] for g in big]
            off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64); ro = np.concatenate(lists).astype(np.uint32)
            bb = ReadSet.from_strings([rs.get(int(x[0]))[0] for x in lists])
            pp = polish_params(iters=2, k=13, w=20, tile_depth=4, band=0, trim=2)
            got = api._polish1(bb, dev, off, pp, read_order=ro)
            want = fresh._polish1(bb, dev2, off, pp, read_order=ro)
            assert got[0] == want[0] and np.array_equal(got[1], want[1])
        finally:
            dev.release(); dev2.release()


def test_argument_errors():
    sp = synth.make_species(2, 400, 0.12, seed=44)
    with runtime.new_api() as api:
        rs, _ = _sample(api, sp, 300, 9)
        n = rs.n
        prm = cluster_params(k=13, w=20, p_shared=select_p_table(13, 20))
        for seg in ([0, 200, 100, n], [0, 100, n - 1], [1, 100, n]):
            with pytest.raises(NgsidError) as e:
                api.cluster_greedy_segmented(rs, prm, seg)
            assert e.value.code == -2
        # k = 21: 63 bits of code, one bit of segment number -> two segments are the limit
        p21 = cluster_params(k=21, w=30, p_shared=select_p_table(21, 30))
        api.cluster_greedy_segmented(rs, p21, [0, 100, n])
        with pytest.raises(NgsidError) as e:
            api.cluster_greedy_segmented(rs, p21, [0, 100, 200, n])
        assert e.value.code == -2
        # k = 15: 19 bits
        p15 = cluster_params(k=15, w=50, p_shared=select_p_table(15, 50))
        seg = np.full((1 << 19) + 2, n, dtype=np.uint64); seg[0] = 0
        with pytest.raises(NgsidError) as e:
            api.cluster_greedy_segmented(rs, p15, seg)
        assert e.value.code == -2


def _centers(res):
    return [(c[0], c[1], c[2], c[3], list(c[4])) for c in res["centers"]]


@pytest.mark.parametrize("long_sample,lanes", [(False, 1), (True, 1), (False, 2)])
def test_run_hot_path_samples_equals_run_hot_path_per_sample(gpu_api, monkeypatch, long_sample, lanes):
    """membership, drafts, polished strings, n_reads and groups; with one sample of reads above 3 000 bases in the batch the other samples keep their 64-column band"""
    api = gpu_api
    sp = synth.make_species(4, 600, 0.12, seed=45)
    parts = [_sample(api, sp, n, 60 + i, abundance=ab) for i, (n, ab) in enumerate([(500, None), (260, [0.5, 0.3, 0.15, 0.05]), (700, [0.1, 0.1, 0.4, 0.4])])]
    if long_sample:
        parts.insert(1, _sample(api, synth.make_species(2, 3300, 0.12, seed=46), 120, 70, mu=16.0))
        assert int(np.diff(parts[1][0].off.astype(np.int64)).max()) > 3000
    rs, seg = _concat([p[0] for p in parts]); score = np.concatenate([p[1] for p in parts])
    kw = dict(k=13, w=20, abundance_ratio=0.08, racon_iter=2, p_shared=select_p_table(13, 20))
    monkeypatch.setattr(_capi, "LANE_MIN_READS", 0)
    saved = api.lanes
    dev = api.upload_reads(rs)
    try:
        api.lanes = 1
        want = []
        for (x, sc) in parts:
            d = api.upload_reads(x)
            try: want.append(pipeline.run_hot_path(api, d, sc, acc_rank=np.arange(x.n, dtype=np.uint32), **kw))
            finally: d.release()
        api.lanes = lanes
        got = pipeline.run_hot_path_samples(api, dev, score, seg, acc_rank=np.arange(rs.n, dtype=np.uint32), **kw)
        if lanes > 1: assert len(api.contexts()) >= 2
    finally:
        api.lanes = saved
        dev.release()
    assert len(got) == len(parts)
    for s, (g, w_) in enumerate(zip(got, want)):
        assert np.array_equal(g["rep_of"], w_["rep_of"]) and np.array_equal(g["status"], w_["status"]) and np.array_equal(g["counters"], w_["counters"]), "sample %d: membership" % s
        assert len(w_["centers"]) >= 2 and _centers(g) == _centers(w_), "sample %d: centres" % s


def test_strand_aware_is_refused(gpu_api):
    rs = _fixed(["ACGT" * 30] * 4)
    with pytest.raises(ValueError):
        pipeline.run_hot_path_samples(gpu_api, rs, np.ones(4), [0, 2, 4], strand_aware=True, p_shared=select_p_table(13, 20))


def _files(folder):
    import os
    out = {}
    for root, _, fs in os.walk(folder):
        for f in fs:
            out[os.path.relpath(os.path.join(root, f), folder)] = open(os.path.join(root, f), "rb").read()
    return out


def test_cli_fastq_dir_equals_one_run_per_file(gpu_api, tmp_path):
    """--fastq_dir over three files: per sample folder the files of the single run, byte for byte (sorted.fastq, the TSVs, consensus_reference_*, reads_to_consensus_*,
    racon_cl_id_*/ with every iteration and PAF, logfile.txt)"""
    import os, shutil
    from oracle_lib import GOLD
    from ngspeciesid_amd.cli import cli
    d = tmp_path / "in"; d.mkdir()
    shutil.copy(os.path.join(GOLD, "sample_h1.fastq"), str(d / "h1.fastq"))
    sp = synth.make_species(3, 650, 0.12, seed=47)
    synth.reads_to_fastq(synth.make_reads(sp, 900, mu=15.0, seed=48, rc_fraction=0.3), str(d / "s_a.fastq"), prefix="a")
    synth.reads_to_fastq(synth.make_reads(sp, 350, mu=14.0, seed=49, abundance=[0.7, 0.2, 0.1]), str(d / "s_b.fq"), prefix="b")
    flags = ["--t", "1", "--consensus", "--racon", "--racon_iter", "2"]
    cli(["--ont", "--fastq_dir", str(d), "--outfolder", str(tmp_path / "batch")] + flags)
    for f in sorted(os.listdir(str(d))):
        cli(["--ont", "--fastq", str(d / f), "--outfolder", str(tmp_path / "single" / os.path.splitext(f)[0])] + flags)
    got, want = _files(str(tmp_path / "batch")), _files(str(tmp_path / "single"))
    assert sorted(got) == sorted(want)
    for name in ("h1", "s_a", "s_b"):
        mine = [k for k in want if k.startswith(name + os.sep)]
        assert {name + "/sorted.fastq", name + "/final_clusters.tsv", name + "/final_cluster_origins.tsv", name + "/logfile.txt"} <= set(mine)
        assert any("consensus_reference_" in k for k in mine) and any("reads_to_consensus_" in k for k in mine)
        assert any("racon_cl_id_" in k and k.endswith("read_alignments_it_1.paf") for k in mine) and any(k.endswith("racon_polished_it_1.fasta") for k in mine)
    for k in want:
        assert got[k] == want[k], k


def test_cli_fastq_dir_needs_t1(tmp_path, caplog):
    import logging
    from ngspeciesid_amd.cli import cli
    d = tmp_path / "in"; d.mkdir()
    with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as e:
        cli(["--ont", "--fastq_dir", str(d), "--outfolder", str(tmp_path / "o"), "--consensus", "--racon"])
    assert e.value.code not in (0, None) and "--fastq_dir requires --t 1" in caplog.text
