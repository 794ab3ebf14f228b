"""Read sets shared by tests/test_phase_cpu.py, tests/test_gpu_phase.py and tools/phase_sweep.py.  Test infrastructure - never imported by the product."""
import numpy as np
from ngspeciesid_amd import synth
from ngspeciesid_amd._capi import ReadSet
from ngspeciesid_amd.hostutil import subset_reads
from ngspeciesid_amd.ptable import select_p_table

SPLIT_SEED = 500          # the read set of the pipeline tests (the seeds tried are listed in tests/test_phase_cpu.py)
KW = dict(k=13, w=20, abundance_ratio=0.05, racon_iter=2, band=0, p_shared=select_p_table(13, 20))


def enc(s):
    return np.frombuffer(s.encode(), dtype=np.uint8)


def concat(sets):
    seq = np.concatenate([s.seq for s in sets]); qual = np.concatenate([s.qual for s in sets])
    lens = np.concatenate([np.diff(s.off.astype(np.int64)) for s in sets])
    off = np.zeros(len(lens) + 1, dtype=np.uint64); off[1:] = np.cumsum(lens)
    return ReadSet(seq, qual, off)


def reads_of(template, n, mu, seed, rc_fraction=0.5):
    rd = synth.make_reads([enc(template)], n, mu=mu, seed=seed, rc_fraction=rc_fraction)
    return ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64))


def variant(template, snps, indel_at=None):
    """the template with another base at every position of snps (the same length: positions stay comparable) and, with indel_at, that base removed"""
    a = list(template)
    for p in snps: a[p] = "ACGT"[("ACGT".index(a[p]) + 2) % 4]
    if indel_at is not None: del a[indel_at]
    return "".join(a)


def with_homopolymers(template, runs):
    """the template with a run of one letter written over it at every (position, length) of runs"""
    a = list(template)
    for x, (p, n) in enumerate(runs):
        a[p:p + n] = "ACGT"[x % 4] * n
    return "".join(a)


def pooled(templates, n_each, mu, seed):
    """n_each reads of every template, mixed strands -> (read set, template of every read)"""
    if isinstance(n_each, int): n_each = [n_each] * len(templates)
    sets = [reads_of(t, n, mu, seed + 17 * i) for i, (t, n) in enumerate(zip(templates, n_each))]
    return concat(sets), np.repeat(np.arange(len(templates)), [s.n for s in sets])


def score_ordered(api, rs, origin):
    """the reads the pipeline sees: quality-filtered and in score order, as the CLI hands them over -> (read set, score, origin)"""
    score, err, keep = api.score_reads(rs, 13, 7.0)
    idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
    return subset_reads(rs, idx), score[idx], origin[idx]


def three_templates(seed=5):
    """two haplotypes of a 400-base amplicon that differ at positions 60, 200 and 340, and one unrelated species"""
    a = synth.make_species(1, 400, 0.0, indel=0.0, seed=seed)[0].tobytes().decode()
    other = synth.make_species(1, 400, 0.0, indel=0.0, seed=seed + 1000)[0].tobytes().decode()
    return [a, variant(a, (60, 200, 340)), other]
