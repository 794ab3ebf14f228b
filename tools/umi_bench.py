#!/usr/bin/env python3
"""ngsid_umi_pairs on one GPU: the whole call and its kernels, against what the library could do before for the same question (Api.near_pairs, one strand), and the
UMI mode end to end.

Seeded synthetic keys: molecules with a random key of --key_len letters, --reads keys per molecule, every letter of a key substituted, deleted or followed by an
insertion with probability --error / 3 each; max_dist --max_dist, seed_len by the policy of ngspeciesid_amd/umi.py for keys of that length.

    python tools/umi_bench.py                               # appends to profiles/umi.txt
    python tools/umi_bench.py --out /tmp/u.txt --keys 100000 --no_end_to_end

Per key count one JSON line: keys, pairs found; the whole Api.umi_pairs call (the count call and the fill call: host clock, median of --repeats after one warm-up) and
the fill call alone; the HIP-event times of k_umi_keys, the index sort, k_umi_ranges, k_umi_join, k_umi_short and the ordering sort of one profiled fill call; the candidates that
went through the Myers column and candidates per second over the time of k_umi_join.  The yardstick is measured in the same run where it fits: Api.near_pairs
(both_strands=False) on the same keys up to --near_max keys - the two results are compared, and where they differ a sample of the pairs only one side reports is
checked against tests/variants_reference.py -, and beyond that (or where it did not return the same pairs) its time at the largest key count at which it did, scaled by
the number of pairs and labelled extrapolated.

The end-to-end line: umi.run on --molecules x --reads reads of about 750 bases (an amplicon of synth.make_reads between exact flanks, UMIs with the key error), the
stage times of extraction, bins, consensus and polishing; beside it, for scale only, pipeline.run_hot_path on the same reads."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def noisy_copies(rng, roots, copies, error):
    """roots int [m, L] (codes 0 .. 3) -> m * copies strings, copy c of root r at r * copies + c: per letter a substitution, a deletion or an insertion behind it"""
    m, L = roots.shape
    base = np.repeat(roots, copies, axis=0)
    u = rng.random(base.shape)
    sub = u < error / 3; dele = (u >= error / 3) & (u < 2 * error / 3); ins = (u >= 2 * error / 3) & (u < error)
    base = np.where(sub, (base + rng.integers(1, 4, base.shape)) % 4, base)
    emit = np.where(dele, 0, np.where(ins, 2, 1))
    flat = np.repeat(base.reshape(-1), emit.reshape(-1))
    second = np.zeros(len(flat), dtype=bool)
    ends = np.cumsum(emit.reshape(-1))
    second[ends[ins.reshape(-1)] - 1] = True                       # the inserted letter stands behind its letter
    flat = np.where(second, rng.integers(0, 4, len(flat)), flat)
    text = ACGT[flat].tobytes()
    off = np.concatenate(([0], np.cumsum(emit.sum(axis=1))))
    return [text[off[i]:off[i + 1]].decode() for i in range(m * copies)]


def make_keys(n, reads, key_len, error, seed):
    rng = np.random.default_rng(seed)
    keys = noisy_copies(rng, rng.integers(0, 4, (max(n // reads, 1), key_len)), reads, error)[:n]
    return [keys[i] for i in rng.permutation(len(keys))]


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


def pairs_line(a, api, n, near_rate):
    from ngspeciesid_amd._capi import ReadSet
    from ngspeciesid_amd import umi
    keys = make_keys(n, a.reads, a.key_len, a.error, 7)
    rs = ReadSet.from_strings(keys)
    half = a.key_len // 2
    g = umi.seed_len(umi.Design("A", "C", "G", "T", half, a.len_slack), a.max_dist)      # the policy's seed length: every key of at least 2 (half - len_slack) letters is seedable
    call_s, found = timed(lambda: api.umi_pairs(rs, a.max_dist, g), a.repeats)
    nfound = len(found[0])
    fill_s, again = timed(lambda: api.umi_pairs(rs, a.max_dist, g, cap=nfound), a.repeats)
    assert all(np.array_equal(x, y) for x, y in zip(found, again))
    prof = kernels(api, lambda: api.umi_pairs(rs, a.max_dist, g, cap=nfound))
    ms = lambda k: round(prof.get(k, (0, 0.0))[1], 3)
    cand = int(prof.get("umi_candidates", (0, 0.0))[0])
    npairs = n * (n - 1) // 2
    row = dict(keys=n, distinct_keys=len(set(keys)), key_len=a.key_len, reads_per_molecule=a.reads, error=a.error, max_dist=a.max_dist, seed_len=g, all_pairs=int(npairs), found=int(nfound),
               umi_pairs_call_s=round(call_s, 5), umi_pairs_fill_call_s=round(fill_s, 5), k_umi_check_ms=ms("k_umi_check"), k_umi_keys_ms=ms("k_umi_keys"), k_umi_sort_ms=ms("k_umi_sort"),
               k_umi_ranges_ms=ms("k_umi_ranges"), k_umi_join_ms=ms("k_umi_join"), k_umi_short_ms=ms("k_umi_short"), k_umi_order_ms=ms("k_umi_order"), candidates_verified=cand,
               verifications_per_s=round(cand / (ms("k_umi_join") * 1e-3)) if ms("k_umi_join") else None)
    if n <= a.near_max:
        near_s, near = timed(lambda: api.near_pairs(rs, a.max_dist, both_strands=False), a.repeats)
        agree = all(np.array_equal(x, y) for x, y in zip(near[:3], found))
        nprof = kernels(api, lambda: api.near_pairs(rs, a.max_dist, both_strands=False, cap=len(near[0])))
        tiles_ms = nprof.get("k_near_tiles", (0, 0.0))[1]
        row.update(near_pairs_call_s=round(near_s, 5), k_near_tiles_ms=round(tiles_ms, 3), near_pairs_over_umi_pairs_call=round(near_s / call_s, 1), near_pairs_found=int(len(near[0])), near_pairs_agrees=bool(agree))
        if not agree:                                                  # which side is right: a sample of the pairs only one of them reports, against the plain reference
            import variants_reference as ref
            code = lambda r: r[0].astype(np.int64) * n + r[1].astype(np.int64)
            cu, cn = code(found), code(near)
            only_u, only_n = np.setdiff1d(cu, cn)[:a.ref_pairs], np.setdiff1d(cn, cu)[:a.ref_pairs]
            within = lambda cs: int(sum(ref.ed(keys[int(c) // n], keys[int(c) % n]) <= a.max_dist for c in cs))
            row.update(only_umi_pairs=int(len(np.setdiff1d(cu, cn))), only_near_pairs=int(len(np.setdiff1d(cn, cu))), only_umi_pairs_checked=int(len(only_u)), only_umi_pairs_within_by_reference=within(only_u),
                       only_near_pairs_checked=int(len(only_n)), only_near_pairs_within_by_reference=within(only_n))
        if agree: near_rate = (near_s / npairs, tiles_ms / npairs)
    if (n > a.near_max or not row.get("near_pairs_agrees", True)) and near_rate is not None:      # from the largest key count at which Api.near_pairs ran and gave the same pairs
        row.update(near_pairs_call_s_extrapolated=round(near_rate[0] * npairs, 2), k_near_tiles_ms_extrapolated=round(near_rate[1] * npairs, 1),
                   near_pairs_over_umi_pairs_call_extrapolated=round(near_rate[0] * npairs / call_s, 1))
    return row, near_rate


def make_read_set(a):
    """-> (flanks, read set): molecules x reads reads, flank - UMI - flank - amplicon - reverse complement of (flank - UMI - flank), 30 % reverse-complemented"""
    from ngspeciesid_amd import synth
    from ngspeciesid_amd._capi import ReadSet
    import demux_reference as dr
    flanks = dr.make_tags(4, length=20, min_dist=8, seed=17)
    rng = np.random.default_rng(3)
    n = a.molecules * a.reads
    half = a.key_len // 2
    uf = noisy_copies(rng, rng.integers(0, 4, (a.molecules, half)), a.reads, a.error)
    ur = noisy_copies(rng, rng.integers(0, 4, (a.molecules, half)), a.reads, a.error)
    sp = synth.make_species(a.templates, a.amplicon, 0.15, seed=5)
    # molecule m is a copy of template m % templates; synth.make_reads deals its reads to the species at random, so the reads of a species are dealt to its molecules in turn
    rd = synth.make_reads(sp, n, mu=a.mu, seed=9)
    seq, qual, off, species = rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy(), rd["species"].numpy()
    slots = {t: [m * a.reads + c for m in range(t, a.molecules, a.templates) for c in range(a.reads)] for t in range(a.templates)}
    parts, quals = [], []
    for i in range(n):
        t = int(species[i])
        if not slots[t]: continue
        k = slots[t].pop()
        head = (flanks[0] + uf[k] + flanks[1]).encode(); tail = dr.revcomp(flanks[2] + ur[k] + flanks[3]).encode()
        s = head + seq[off[i]:off[i + 1]].tobytes() + tail
        q = b"I" * len(head) + qual[off[i]:off[i + 1]].tobytes() + b"I" * len(tail)
        if rng.random() < 0.3:
            s = dr.revcomp(s.decode()).encode(); q = q[::-1]
        parts.append(s); quals.append(q)
    ro = np.zeros(len(parts) + 1, dtype=np.uint64); ro[1:] = np.cumsum([len(s) for s in parts])
    return flanks, ReadSet(np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), np.frombuffer(b"".join(quals), dtype=np.uint8).copy(), ro)


def end_to_end_line(a, api):
    from ngspeciesid_amd import umi, pipeline
    from ngspeciesid_amd.hostutil import subset_reads
    from ngspeciesid_amd.ptable import select_p_table
    flanks, rs = make_read_set(a)
    design = umi.Design(*flanks, umi_len=a.key_len // 2, len_slack=a.len_slack)
    T = {}
    t0 = time.perf_counter()
    res = umi.run(api, rs, design, max_dist=a.max_dist, min_reads=3, racon_iter=3, timings=T)
    total = time.perf_counter() - t0
    row = dict(end_to_end=True, reads=int(rs.n), mean_read_len=int(len(rs.seq) / max(rs.n, 1)), molecules=a.molecules, templates=a.templates, distinct_keys=len(res["bins"]["umis"]),
               key_pairs=res["bins"]["n_pairs"], bins=len(res["bins"]["centroids"]), bins_with_consensus=len(res["kept"]), reads_ok=int((res["status"] == umi.ST_OK).sum()),
               umi_run_s=round(total, 3), **{k + "_s": round(v, 3) for k, v in T.items()})
    # for scale only: the clustering pipeline on the same reads (it joins the molecules of a template)
    score, err, keep = api.score_reads(rs, 13, 7.0)
    idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
    sub = subset_reads(rs, idx)
    t0 = time.perf_counter()
    hot = pipeline.run_hot_path(api, sub, score[idx], acc_rank=np.arange(sub.n, dtype=np.uint32), k=13, w=20, abundance_ratio=0.02, racon_iter=3, p_shared=select_p_table(13, 20))
    row.update(run_hot_path_s=round(time.perf_counter() - t0, 3), run_hot_path_centres=len(hot["centers"]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "umi.txt")); ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--keys", default="20000,100000,1000000", help="key counts, comma separated, ascending"); ap.add_argument("--near_max", type=int, default=100000, help="Api.near_pairs is run up to this many keys and extrapolated beyond")
    ap.add_argument("--key_len", type=int, default=36); ap.add_argument("--reads", type=int, default=20); ap.add_argument("--error", type=float, default=0.05); ap.add_argument("--max_dist", type=int, default=3); ap.add_argument("--len_slack", type=int, default=2); ap.add_argument("--ref_pairs", type=int, default=2000, help="where the two calls disagree: pairs of either side checked against the plain reference")
    ap.add_argument("--molecules", type=int, default=10000); ap.add_argument("--templates", type=int, default=10); ap.add_argument("--amplicon", type=int, default=634); ap.add_argument("--mu", type=float, default=17.0)
    ap.add_argument("--no_end_to_end", action="store_true"); ap.add_argument("--no_pairs", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "umi_bench.py measures on a GPU"
    from ngspeciesid_amd import runtime
    api = runtime.get_api()
    lines = ["# tools/umi_bench.py --key_len %d --reads %d --error %g --max_dist %d --repeats %d" % (a.key_len, a.reads, a.error, a.max_dist, a.repeats)]
    near_rate = None
    if not a.no_pairs:
        for n in (int(x) for x in a.keys.split(",")):
            row, near_rate = pairs_line(a, api, n, near_rate)
            lines.append(json.dumps(row)); print(lines[-1], flush=True)
    if not a.no_end_to_end:
        lines.append(json.dumps(end_to_end_line(a, api))); print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print(lines[0])


if __name__ == "__main__":
    main()
