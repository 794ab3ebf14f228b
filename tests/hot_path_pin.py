"""The pin of pipeline.run_hot_path / run_hot_path_samples on the reference's sample_h1 reads, shared by test_hot_path_pin_cpu.py (oracle) and test_gpu_hot_path_pin.py
(HIP library).  The expected sequences (tests/golden/sample_h1_consensus_oracle.json, key `shipped`) were recorded from the files the COMMAND LINE writes - fastpath.py, a
separate implementation of the same flow - so this is not a comparison of the array driver with itself."""
import json, os
import numpy as np
from ngspeciesid_amd import fastio, pipeline
from ngspeciesid_amd._capi import ReadSet
from ngspeciesid_amd.hostutil import subset_reads
from ngspeciesid_amd.ptable import select_p_table
from oracle_lib import GOLD

KW = dict(k=13, w=20, abundance_ratio=0.1, racon_iter=3, node_cap=0, p_shared=select_p_table(13, 20))


def sorted_reads(api):
    """the reads of sample_h1.fastq the command line clusters, in its order: quality-filtered, by descending score (stable) -> (ReadSet, score)"""
    rs = fastio.read_fastq(os.path.join(GOLD, "sample_h1.fastq"))[1]
    score, _, keep = api.score_reads(rs, 13, 7.0)
    idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
    sub = subset_reads(rs, idx)
    assert sub.n == 274 and int(np.diff(sub.off.astype(np.int64)).max()) == 725
    return sub, score[idx]


def check_pinned(res):
    """res: a run_hot_path result on sorted_reads() with KW"""
    gold = json.load(open(os.path.join(GOLD, "sample_h1_consensus_oracle.json")))["shipped"]
    assert len(res["centers"]) == 1
    n_reads, c_id, draft, polished, groups = res["centers"][0]
    assert (n_reads, c_id) == (253, gold["c_id"]) and c_id == 17
    assert draft == gold["draft"]
    assert polished == gold["it2"][1]
    assert polished == gold["consensus_fasta"].split("\n")[1]


def check_single(api):
    sub, score = sorted_reads(api)
    res = pipeline.run_hot_path(api, sub, score, acc_rank=np.arange(sub.n, dtype=np.uint32), **KW)
    check_pinned(res)
    return res


def check_samples(api, single):
    """three segments - the reads, nothing, the reads again; single: the run_hot_path result of check_single"""
    sub, score = sorted_reads(api)
    lens = np.diff(sub.off.astype(np.int64))
    off = np.zeros(2 * sub.n + 1, dtype=np.uint64); off[1:] = np.cumsum(np.concatenate([lens, lens]))
    rs = ReadSet(np.concatenate([sub.seq, sub.seq]), np.concatenate([sub.qual, sub.qual]), off)
    seg = [0, sub.n, sub.n, 2 * sub.n]
    sc = np.concatenate([score, score]); acc = np.arange(rs.n, dtype=np.uint32)
    out = pipeline.run_hot_path_samples(api, rs, sc, seg, acc_rank=acc, **KW)
    assert len(out) == 3
    for s in (0, 2):
        check_pinned(out[s])
        assert out[s]["centers"] == single["centers"] and np.array_equal(out[s]["rep_of"], single["rep_of"])
    assert out[1]["centers"] == [] and len(out[1]["rep_of"]) == 0
    only = pipeline.run_hot_path_samples(api, rs, sc, seg, acc_rank=acc, do_consensus=False, **KW)
    assert len(only) == 3 and all(o["centers"] == [] for o in only)
    assert all(np.array_equal(o["rep_of"], w["rep_of"]) for o, w in zip(only, out))
