#!/usr/bin/env python3
"""ngsid_near_pairs on one GPU: the whole call and its kernels, against the edit-distance aligner the library had before on a sample of the same pairs, and against
the numpy reference of the tests.

Two workloads of seeded synthetic consensuses (families: a random root, every member with --divergence / 2 substitutions, so two members of a family are --divergence
apart and all sequences have --length bases: no pair is removed by the length bound):
    96 samples x 30 consensuses (30 families, one member per sample) = 2 880 sequences, and 20 000 sequences (200 families of 100).

    python tools/variants_bench.py                       # appends to profiles/variants.txt
    python tools/variants_bench.py --out /tmp/v.txt --configs 30x96

Per workload one JSON line: sequences, candidate pairs and pair-strands (every pair on two strands), pairs found at --max_dist; the whole Api.near_pairs call (the count
call and the fill call: host clock, median of --repeats after one warm-up) and the fill call alone; the HIP-event time of k_near_pack and k_near_tiles of one profiled
fill call; pair-strands per second over the time of k_near_tiles.  The number to hold it against is measured in the same run: the `distance` output of
Api.ed_align_batch - what the parent commit can do for these pairs - on a fixed random sample of --sample of the same pairs, forward strand: its call time and the time
of its kernel (the profiling line k_ed_align).  Its figure for the whole workload is that time scaled by pair-strands / sample and is labelled extrapolated.  The numpy
reference (tests/variants_reference.py) is timed on --ref_pairs pairs, both strands; its figure for the whole workload is extrapolated the same way.

The wide leg (--wide K[,K...], e.g. --wide 63,127,255): ngsid_near_pairs_wide at each bound K on the same two shapes, with families whose members are (32 + K) / 2 edits
apart on average, so that the distances within a family fall between 32 and K - pairs the one-word band cannot join.  Per (workload, K) one JSON line: the whole
Api.near_pairs_wide call and the fill call alone, the HIP-event time of k_near_tiles_wide, pair-strands per second; beside them, on the same set, the one-word
k_near_tiles at max_dist 31 (what a run had to settle for before) and Api.ed_align_batch on --sample of the same pairs with its extrapolation, as in the first leg.
    python tools/variants_bench.py --wide 63,127,255"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_families(n_families, per, length, divergence, seed):
    """member m of family f is sequence m * n_families + f: a sample holds one member of every family"""
    rng = np.random.default_rng(seed)
    roots = rng.integers(0, 4, (n_families, length))
    seqs = []
    for _ in range(per):
        for f in range(n_families):
            hit = rng.random(length) < divergence / 2
            seqs.append(ACGT[np.where(hit, (roots[f] + rng.integers(1, 4, length)) % 4, roots[f])].tobytes().decode())
    return seqs


def kernels(api, fn):
    api.profile_enable(True); api.profile_read()
    fn()
    prof = api.profile_read()[0]
    api.profile_enable(False)
    return prof


def timed(fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter(); out = fn(); t.append(time.perf_counter() - t0)
    return float(np.median(t)), out


def wide_leg(a, api, bounds):
    """one JSON line per (workload, wide bound)"""
    from ngspeciesid_amd._capi import ReadSet, NEAR_MAX_DIST
    import variants_reference as ref
    lines = ["# tools/variants_bench.py --wide %s --length %d --repeats %d --sample %d" % (",".join(str(k) for k in bounds), a.length, a.repeats, a.sample)]
    for cfg in a.configs.split(","):
        nf, per = (int(x) for x in cfg.split("x"))
        for K in bounds:
            divergence = (32 + K) / 2.0 / a.length
            seqs = make_families(nf, per, a.length, divergence, 7)
            rs = ReadSet.from_strings(seqs); n = len(seqs)
            npairs = n * (n - 1) // 2; strands = 2 * npairs
            call_s, found = timed(lambda: api.near_pairs_wide(rs, K), a.repeats)
            nfound = len(found[0])
            fill_s, again = timed(lambda: api.near_pairs_wide(rs, K, cap=nfound), a.repeats)
            assert all(np.array_equal(x, y) for x, y in zip(found, again))
            prof = kernels(api, lambda: api.near_pairs_wide(rs, K, cap=nfound))
            tiles_ms, pack_ms = prof.get("k_near_tiles_wide", (0, 0.0))[1], prof.get("k_near_pack", (0, 0.0))[1]
            # the one-word kernel at its own largest bound on the same set: what it costs, and how few of these pairs it finds
            narrow = api.near_pairs(rs, NEAR_MAX_DIST)
            nprof = kernels(api, lambda: api.near_pairs(rs, NEAR_MAX_DIST, cap=len(narrow[0])))
            narrow_ms = nprof.get("k_near_tiles", (0, 0.0))[1]
            # the yardstick: the same pairs through the edit-distance aligner, forward strand, a fixed random sample
            rng = np.random.default_rng(11)
            ns = min(a.sample, npairs)
            qi = rng.integers(0, n, ns); ti = (qi + rng.integers(1, n, ns)) % n
            ed_s, ed_out = timed(lambda: api.ed_align_batch(rs, rs, qi, ti), a.repeats)
            eprof = kernels(api, lambda: api.ed_align_batch(rs, rs, qi, ti))
            ed_ms = sum(v[1] for k, v in eprof.items() if k.startswith("k_ed_align"))
            within = api.ed_within_wide(rs, rs, qi, ti, K, both_strands=False)[0]
            nref = min(a.ref_pairs, ns)
            same = [p for p in range(ns) if qi[p] % nf == ti[p] % nf][:nref]              # pairs of one family: the ones with a distance to compare
            want = ref.ed_within(seqs, seqs, qi[same], ti[same], K)
            both = api.ed_within_wide(rs, rs, qi[same], ti[same], K)
            assert np.array_equal(both[0], want[0]) and np.array_equal(both[1], want[1])
            lines.append(json.dumps(dict(config=cfg, sequences=n, pairs=int(npairs), pair_strands=int(strands), wide_max_dist=int(K), family_divergence=round(divergence, 4),
                                         found=int(nfound), found_beyond_31=int((found[2] > NEAR_MAX_DIST).sum()),
                                         near_pairs_wide_call_s=round(call_s, 5), near_pairs_wide_fill_call_s=round(fill_s, 5), k_near_tiles_wide_ms=round(tiles_ms, 3), k_near_pack_ms=round(pack_ms, 3),
                                         pair_strands_per_s=round(strands / (tiles_ms * 1e-3)) if tiles_ms else None,
                                         one_word_found_at_31=int(len(narrow[0])), one_word_k_near_tiles_ms=round(narrow_ms, 3),
                                         wide_over_one_word_kernel=round(tiles_ms / narrow_ms, 1) if narrow_ms else None,
                                         ed_align_sample_pairs=int(ns), ed_align_call_s=round(ed_s, 5), ed_align_kernel_ms=round(ed_ms, 3),
                                         ed_align_whole_kernel_s_extrapolated=round(ed_ms * 1e-3 * strands / ns, 3) if ed_ms else None,
                                         ed_align_whole_call_s_extrapolated=round(ed_s * strands / ns, 3),
                                         kernel_ratio_extrapolated=round((ed_ms * strands / ns) / tiles_ms, 1) if ed_ms and tiles_ms else None,
                                         sample_within_wide_max_dist=int((within >= 0).sum()), sample_ed_align_within_wide_max_dist=int((ed_out[0] <= K).sum()),
                                         reference_pairs_checked=len(same), reference_distances=[int(x) for x in want[0]])))
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variants.txt")); ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--length", type=int, default=650); ap.add_argument("--divergence", type=float, default=0.05); ap.add_argument("--max_dist", type=int, default=31)
    ap.add_argument("--sample", type=int, default=100000); ap.add_argument("--ref_pairs", type=int, default=8)
    ap.add_argument("--configs", default="30x96,200x100", help="families x members, comma separated")
    ap.add_argument("--wide", default="", help="run the wide leg instead: the bounds of ngsid_near_pairs_wide to measure, comma separated (e.g. 63,127,255)")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "variants_bench.py measures on a GPU"
    from ngspeciesid_amd import runtime
    from ngspeciesid_amd._capi import ReadSet
    import variants_reference as ref
    api = runtime.get_api()
    if a.wide:
        lines = wide_leg(a, api, [int(k) for k in a.wide.split(",")])
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
        print(lines[0])
        return
    lines = ["# tools/variants_bench.py --length %d --divergence %g --max_dist %d --repeats %d --sample %d" % (a.length, a.divergence, a.max_dist, a.repeats, a.sample)]
    for cfg in a.configs.split(","):
        nf, per = (int(x) for x in cfg.split("x"))
        seqs = make_families(nf, per, a.length, a.divergence, 7)
        rs = ReadSet.from_strings(seqs); n = len(seqs)
        npairs = n * (n - 1) // 2; strands = 2 * npairs
        call_s, found = timed(lambda: api.near_pairs(rs, a.max_dist), a.repeats)
        nfound = len(found[0])
        fill_s, again = timed(lambda: api.near_pairs(rs, a.max_dist, cap=nfound), a.repeats)
        assert all(np.array_equal(x, y) for x, y in zip(found, again))
        prof = kernels(api, lambda: api.near_pairs(rs, a.max_dist, cap=nfound))
        tiles_ms, pack_ms = prof.get("k_near_tiles", (0, 0.0))[1], prof.get("k_near_pack", (0, 0.0))[1]
        # the yardstick: the same pairs through the edit-distance aligner, forward strand, a fixed random sample
        rng = np.random.default_rng(11)
        ns = min(a.sample, npairs)
        qi = rng.integers(0, n, ns); ti = (qi + rng.integers(1, n, ns)) % n
        ed_s, ed_out = timed(lambda: api.ed_align_batch(rs, rs, qi, ti), a.repeats)
        eprof = kernels(api, lambda: api.ed_align_batch(rs, rs, qi, ti))
        ed_ms = sum(v[1] for k, v in eprof.items() if k.startswith("k_ed_align"))
        within = api.ed_within(rs, rs, qi, ti, a.max_dist, both_strands=False)[0]
        # (ed_align_batch aligns the query inside the target with free target ends, so its distance is a lower bound of the global one and equal for equal lengths up to end gaps)
        nref = min(a.ref_pairs, ns)
        t0 = time.perf_counter()
        want = ref.ed_within(seqs, seqs, qi[:nref], ti[:nref], a.max_dist)
        tref = time.perf_counter() - t0
        both = api.ed_within(rs, rs, qi[:nref], ti[:nref], a.max_dist)
        assert np.array_equal(both[0], want[0]) and np.array_equal(both[1], want[1])
        lines.append(json.dumps(dict(config=cfg, sequences=n, pairs=int(npairs), pair_strands=int(strands), max_dist=a.max_dist, found=int(nfound),
                                     near_pairs_call_s=round(call_s, 5), near_pairs_fill_call_s=round(fill_s, 5), k_near_tiles_ms=round(tiles_ms, 3), k_near_pack_ms=round(pack_ms, 3),
                                     k_near_check_ms=round(prof.get("k_near_check", (0, 0.0))[1], 3),
                                     pair_strands_per_s=round(strands / (tiles_ms * 1e-3)) if tiles_ms else None,
                                     ed_align_sample_pairs=int(ns), ed_align_call_s=round(ed_s, 5), ed_align_kernel_ms=round(ed_ms, 3),
                                     ed_align_pair_strands_per_s=round(ns / (ed_ms * 1e-3)) if ed_ms else None,
                                     ed_align_whole_kernel_s_extrapolated=round(ed_ms * 1e-3 * strands / ns, 3) if ed_ms else None,
                                     ed_align_whole_call_s_extrapolated=round(ed_s * strands / ns, 3),
                                     kernel_ratio_extrapolated=round((ed_ms * strands / ns) / tiles_ms, 1) if ed_ms and tiles_ms else None,
                                     sample_within_max_dist=int((within >= 0).sum()), sample_ed_align_within_max_dist=int((ed_out[0] <= a.max_dist).sum()),
                                     reference_pairs=int(nref), reference_s=round(tref, 3), reference_whole_s_extrapolated=round(tref * npairs / max(nref, 1), 1))))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text)
    print(lines[0])


if __name__ == "__main__":
    main()
