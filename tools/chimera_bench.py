#!/usr/bin/env python3
"""ngsid_chimera_model on one GPU: the whole call and both kernels, against the affine aligner on the same pairs and against the numpy reference of the tests.

Two workloads of seeded synthetic consensuses (per sample one family: a random root, every member with --divergence / 2 substitutions; read counts log-normal, so the
abundance skew offers each consensus a different number of parents, both strands each - chimera.model, the pipeline's own pair construction):
    96 samples x 30 consensuses x 650 bases, and one sample x 200 consensuses x 650 bases.

    python tools/chimera_bench.py                       # appends to profiles/chimera.txt
    python tools/chimera_bench.py --out /tmp/c.txt

Per workload one JSON line: pairs, the whole Api.chimera_model call (host clock, median of --repeats after one warm-up), the HIP-event time of k_chimera_profile and
k_chimera_reduce of one profiled run, and the cell rate of k_chimera_profile, 2 n m per pair (two rectangles) over its time.  The number to hold it against is measured
in the same run: Api.sg_align_batch (open 3, ext 1, +2 / -2: the aligner of the reverse-complement step) on the same (query, parent strand) pairs, n m per pair over the
time of its kernels (every profiling line that starts with k_sg_align).  The numpy reference (tests/chimera_reference.py) is timed on --ref_pairs pairs; its figure for
the whole workload is that time scaled by the pair count and is labelled extrapolated."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_samples(n_samples, per, length, divergence, seed):
    rng = np.random.default_rng(seed)
    seqs, sizes = [], []
    for s in range(n_samples):
        root = rng.integers(0, 4, length)
        for _ in range(per):
            hit = rng.random(length) < divergence / 2
            seqs.append(ACGT[np.where(hit, (root + rng.integers(1, 4, length)) % 4, root)].tobytes().decode())
        sizes += np.maximum(rng.lognormal(4.0, 1.2, per).astype(np.int64), 3).tolist()
    return seqs, np.asarray(sizes), np.arange(0, n_samples * per + 1, per)


def kernels(api, fn):
    api.profile_enable(True); api.profile_read()
    fn()
    prof = api.profile_read()[0]
    api.profile_enable(False)
    return prof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chimera.txt")); ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--length", type=int, default=650); ap.add_argument("--divergence", type=float, default=0.1); ap.add_argument("--ref_pairs", type=int, default=24)
    ap.add_argument("--configs", default="96x30,1x200")
    a = ap.parse_args()
    from ngspeciesid_amd import runtime, chimera, classify
    from ngspeciesid_amd._capi import ReadSet, CHIMERA_ROWS
    import chimera_reference as ref
    api = runtime.get_api()
    lines = ["# tools/chimera_bench.py --length %d --divergence %g --repeats %d   (R = %d rows per lane)" % (a.length, a.divergence, a.repeats, CHIMERA_ROWS)]
    for cfg in a.configs.split(","):
        ns, per = (int(x) for x in cfg.split("x"))
        seqs, sizes, so = make_samples(ns, per, a.length, a.divergence, 7)
        qs = ReadSet.from_strings(seqs); both = classify.both_strands(qs)
        offs, parents, gids = [np.zeros(1, np.uint64)], [], []
        for x, y in zip(so[:-1], so[1:]):
            po, pp, pg = chimera.candidates(sizes[x:y])
            offs.append(po[1:] + offs[-1][-1]); parents.append(pp + np.uint32(2 * x)); gids.append(pg + np.int32(x))
        pair_off, pair_parent, pair_gid = np.concatenate(offs), np.concatenate(parents), np.concatenate(gids)
        pair_q = np.repeat(np.arange(len(seqs)), np.diff(pair_off.astype(np.int64)))
        npairs = len(pair_parent); cells = float(npairs) * a.length * a.length
        run = lambda: api.chimera_model(qs, both, pair_off, pair_parent, pair_gid)
        run()
        t = []
        for _ in range(a.repeats):
            t0 = time.perf_counter(); fields = run(); t.append(time.perf_counter() - t0)
        prof = kernels(api, run)
        aln = lambda: api.sg_align_batch(qs, both, pair_q, pair_parent, 3, 1, 2, -2, 13, None)
        aln()
        ta = []
        for _ in range(a.repeats):
            t0 = time.perf_counter(); aln(); ta.append(time.perf_counter() - t0)
        aprof = kernels(api, aln)
        aln_ms = sum(v[1] for k, v in aprof.items() if k.startswith("k_sg_align"))
        nref = min(a.ref_pairs, npairs)
        q_of = pair_q[:nref]; uq = np.unique(q_of)
        t0 = time.perf_counter()
        ref.chimera_model([seqs[q] for q in uq], [both.get(i)[0] for i in range(both.n)], np.concatenate(([0], np.cumsum([int((q_of == q).sum()) for q in uq]))), pair_parent[:nref], pair_gid[:nref])
        tref = time.perf_counter() - t0
        called = chimera.call(fields, [len(s) for s in seqs])
        prof_ms, red_ms = prof.get("k_chimera_profile", (0, 0.0))[1], prof.get("k_chimera_reduce", (0, 0.0))[1]
        lines.append(json.dumps(dict(config=cfg, consensuses=len(seqs), pairs=int(npairs), called=int(called.sum()), call_s=round(float(np.median(t)), 5),
                                     k_chimera_profile_ms=round(prof_ms, 3), k_chimera_reduce_ms=round(red_ms, 3), k_chimera_check_ms=round(prof.get("k_chimera_check", (0, 0.0))[1], 3),
                                     chimera_gcells_per_s=round(2 * cells / (prof_ms * 1e-3) / 1e9, 1) if prof_ms else None,
                                     sg_align_call_s=round(float(np.median(ta)), 5), sg_align_kernels_ms=round(aln_ms, 3), sg_align_kernels={k: round(v[1], 3) for k, v in aprof.items() if k.startswith("k_sg_align")},
                                     sg_align_gcells_per_s=round(cells / (aln_ms * 1e-3) / 1e9, 1) if aln_ms else None,
                                     reference_pairs=int(nref), reference_s=round(tref, 3), reference_whole_s_extrapolated=round(tref * npairs / max(nref, 1), 1))))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
