"""Multi-sample batch mode against the per-sample loop (pipeline.run_hot_path_samples vs a loop of pipeline.run_hot_path), on one GPU.

Synthetic samples at the C3 read profile of bench.py (5 species of 750 bp at 15 % divergence, ONT quality profile mu = 17, k = 13, w = 20, abundance_ratio 0.02, three
polishing iterations); every sample is drawn from the same five amplicons - the case of a demultiplexed run.  Both sides see device-resident reads in score order.

    python tools/multi_sample_bench.py                       # 96 x 10 000 and 24 x 2 000, + 96 x 10 000 with the samples laid end to end
    python tools/multi_sample_bench.py --configs 24x2000 --repeats 5

Per configuration one JSON line: reads/s and ms of both sides (median of --repeats timed runs after one warm-up), dispatches (k_* lines of ngsid_profile_read, one profiled
run each) and the restart rounds of the segmented clustering call.  The results of the two sides are compared sample by sample before anything is timed."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_samples(api, n_samples, n_reads, seed):
    import torch
    from ngspeciesid_amd import synth
    from ngspeciesid_amd._capi import ReadSet
    from ngspeciesid_amd.hostutil import subset_reads
    sp = synth.make_species(5, 750, 0.15, seed=1)
    out = []
    for s0 in range(0, n_samples, 16):                 # 16 samples per generator call
        ns = min(16, n_samples - s0)
        rd = synth.make_reads(sp, ns * n_reads, mu=17.0, seed=seed + s0, device="cuda")
        torch.cuda.synchronize()
        rs = ReadSet(rd["seq"].cpu().numpy(), rd["qual"].cpu().numpy(), rd["off"].cpu().numpy().astype(np.uint64))
        score, err, keep = api.score_reads(rs, 13, 7.0)
        for s in range(ns):
            idx = s * n_reads + np.nonzero(keep[s * n_reads:(s + 1) * n_reads])[0]
            idx = idx[np.argsort(-score[idx], kind="stable")]
            out.append((subset_reads(rs, idx), score[idx]))
        del rd
    torch.cuda.empty_cache()
    return out


def concat(sets):
    from ngspeciesid_amd._capi import ReadSet
    lens = np.concatenate([np.diff(s.off.astype(np.int64)) for s in sets])
    off = np.zeros(len(lens) + 1, dtype=np.uint64); off[1:] = np.cumsum(lens)
    seg = np.zeros(len(sets) + 1, dtype=np.uint64); seg[1:] = np.cumsum([s.n for s in sets])
    return ReadSet(np.concatenate([s.seq for s in sets]), np.concatenate([s.qual for s in sets]), off), seg


def dispatches(prof):
    return int(sum(c for nm, (c, ms) in prof.items() if nm.startswith("k_")))


def timed(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="96x10000,24x2000,96x10000:end_to_end", help="samples x reads per sample[:end_to_end]")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip_loop", action="store_true", help="time the batched side only")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from ngspeciesid_amd import runtime, pipeline
    from ngspeciesid_amd.ptable import select_p_table
    api = runtime.get_api(0)
    kw = dict(k=13, w=20, abundance_ratio=0.02, racon_iter=3, p_shared=select_p_table(13, 20), polish_stop_when_stable=False)
    loop_cache = {}
    for cfg in args.configs.split(","):
        shape, _, order = cfg.partition(":")
        ns, nr = (int(x) for x in shape.split("x"))
        api.set_option("cluster_seg_order", 1 if order == "end_to_end" else 0)
        samples = make_samples(api, ns, nr, seed=1000)
        rs, seg = concat([s[0] for s in samples]); score = np.concatenate([s[1] for s in samples])
        dev = api.upload_reads(rs); devs = [api.upload_reads(s[0]) for s in samples]
        acc = np.arange(rs.n, dtype=np.uint32)
        batched = lambda: pipeline.run_hot_path_samples(api, dev, score, seg, acc_rank=acc, **kw)
        loop = lambda: [pipeline.run_hot_path(api, d, s[1], acc_rank=np.arange(s[0].n, dtype=np.uint32), **kw) for d, s in zip(devs, samples)]
        got = batched()
        line = dict(config=cfg, samples=ns, reads=int(rs.n), item_order=order or "interleaved")
        if not args.skip_loop and shape not in loop_cache:
            want = loop()
            for s, (g, w) in enumerate(zip(got, want)):
                assert np.array_equal(g["rep_of"], w["rep_of"]) and [tuple(c[:4]) for c in g["centers"]] == [tuple(c[:4]) for c in w["centers"]], "sample %d differs" % s
            line["identical_results"] = True
            t, ts = timed(loop, args.repeats)
            api.profile_enable(True); loop(); prof, _ = api.profile_read(); api.profile_enable(False)
            loop_cache[shape] = dict(ms=round(t * 1e3, 1), runs_ms=[round(x * 1e3, 1) for x in ts], reads_per_s=round(rs.n / t), dispatches=dispatches(prof))
        t, ts = timed(batched, args.repeats)
        api.profile_enable(True); batched(); prof, _ = api.profile_read(); api.profile_enable(False)
        line["batched"] = dict(ms=round(t * 1e3, 1), runs_ms=[round(x * 1e3, 1) for x in ts], reads_per_s=round(rs.n / t), dispatches=dispatches(prof),
                               cluster_restart_rounds=int(prof.get("count_cluster_seg_restart_rounds", (0, 0.0))[0]),
                               centres=int(sum(len(g["centers"]) for g in got)))
        if shape in loop_cache:
            line["loop"] = loop_cache[shape]; line["speedup"] = round(loop_cache[shape]["ms"] / line["batched"]["ms"], 2)
        print(json.dumps(line), flush=True)
        dev.release()
        for d in devs: d.release()
    api.set_option("cluster_seg_order", 0)


if __name__ == "__main__":
    main()
