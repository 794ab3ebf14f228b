"""ngsid_demux_locate on one GPU against the host locator in a 16-thread pool.

Seeded synthetic reads: a random 600-base amplicon body per read with a forward tag at the head and the reverse complement of a reverse tag at the tail (24-base
tags, 0 - 3 substitutions each, 0 - 30 random bases outside them; a fifth of the reads reverse-complemented).  "N dual tags" = N forward + N reverse tags, 2 N in all.

    python tools/demux_bench.py                                  # 100 k reads x 24 dual tags and 1 M reads x 96 dual tags; window 150, max_ed 3
    python tools/demux_bench.py --configs 100000x24 --repeats 5

Per configuration one JSON line: the whole demux_locate call (host clock around the call, which ends in a stream synchronise; median of --repeats runs after one
warm-up; device-resident reads) and the k_demux_locate time of one profiled run (ngsid_profile_read: HIP events around the launch).  At the first configuration
only, the comparator: ngsid_host_infix_locate over the same (read end, tag) pairs, called through ctypes (which releases the interpreter lock) from 16 threads, one
run (--host_sample N times it on the first N reads and scales); for the other configurations it is extrapolated from that pair rate and labelled so.

    python tools/demux_bench.py --scan                           # ngsid_demux_scan: the same pools, 2 % of the reads replaced by two-amplicon concatemers

--scan: per configuration one JSON line with the whole demux_scan call of the binding (count call + fill call; median of --repeats), k_demux_scan of one profiled
call (both launches: the count call's and the fill call's) and k_demux_locate in the same process on the same reads.  The yardstick is locate's lane-column rate of
that run (pairs x window columns per second of kernel time) next to the scan's (patterns x read bases per second of kernel time, per launch), and their ratio.
The CPU comparator is the numpy restatement of the definition (tests/demux_scan_reference.py) timed on --scan_host_reads reads and scaled: extrapolated, and labelled so."""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COMP = np.zeros(256, dtype=np.uint8)
for a, b in zip(b"ACGTN", b"TGCAN"):
    COMP[a] = b


def make_pool(n_reads, n_dual, seed, body=600, tag_len=24):
    """-> (ReadSet without qualities, tags [2 * n_dual] as strings)"""
    from ngspeciesid_amd._capi import ReadSet
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    tags = acgt[rng.integers(0, 4, (2 * n_dual, tag_len))]
    j0 = rng.integers(0, 31, n_reads); j1 = rng.integers(0, 31, n_reads)
    lens = j0 + j1 + 2 * tag_len + body
    off = np.zeros(n_reads + 1, dtype=np.uint64); off[1:] = np.cumsum(lens)
    seq = acgt[rng.integers(0, 4, int(off[-1]))]
    s = rng.integers(0, n_dual, n_reads)
    start = off[:-1].astype(np.int64)
    f = tags[s].copy(); r = COMP[tags[n_dual + s][:, ::-1]].copy()
    for t in (f, r):                                                   # up to three substitutions per tag
        for _ in range(3):
            hit = rng.random(n_reads) < 0.5
            pos = rng.integers(0, tag_len, n_reads)
            t[hit, pos[hit]] = acgt[rng.integers(0, 4, int(hit.sum()))]
    cols = np.arange(tag_len)
    seq[(start + j0)[:, None] + cols] = f
    seq[(start + lens - j1 - tag_len)[:, None] + cols] = r
    flip = np.flatnonzero(rng.random(n_reads) < 0.2)
    for i in flip:
        a, b = int(off[i]), int(off[i + 1]); seq[a:b] = COMP[seq[a:b][::-1]]
    return ReadSet(seq, None, off), [t.tobytes().decode() for t in tags]


def with_concatemers(rs, fraction, seed):
    """the read set with `fraction` of its reads replaced by the read followed by another read of the set (a two-amplicon concatemer) -> (ReadSet, number replaced)"""
    from ngspeciesid_amd._capi import ReadSet
    rng = np.random.default_rng(seed)
    n = rs.n; off = rs.off.astype(np.int64); lens = np.diff(off)
    conc = np.flatnonzero(rng.random(n) < fraction)
    seg_read = np.concatenate([np.arange(n), rng.integers(0, n, len(conc))])          # the segments: every read, then the second halves
    seg_owner = np.concatenate([np.arange(n), conc])
    order = np.argsort(seg_owner, kind="stable")                                        # a read's own segment before its second half
    seg_read, seg_owner = seg_read[order], seg_owner[order]
    seg_len = lens[seg_read]
    new_off = np.zeros(n + 1, dtype=np.uint64); new_off[1:] = np.cumsum(np.bincount(seg_owner, weights=seg_len, minlength=n).astype(np.int64))
    dst = np.cumsum(seg_len) - seg_len
    seq = rs.seq[np.repeat(off[seg_read] - dst, seg_len) + np.arange(int(seg_len.sum()))]
    return ReadSet(seq, None, new_off), len(conc)


def revcomp(t):
    return COMP[np.frombuffer(t.encode(), dtype=np.uint8)[::-1]].tobytes().decode()


def scan_bench(api, args):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import demux_scan_reference as sref
    for cfg in args.configs.split(","):
        n, d = (int(x) for x in cfg.split("x"))
        rs, tags = make_pool(n, d, seed=1000 + d)
        rs, n_conc = with_concatemers(rs, 0.02, seed=2000 + d)
        patterns = tags + [revcomp(t) for t in tags]
        bases = int(rs.off[-1])
        dev = api.upload_reads(rs)
        call = lambda: api.demux_scan(dev, patterns, max_ed=args.max_ed)
        hit_off, hits = call()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter(); call(); ts.append(time.perf_counter() - t0)
        api.profile_enable(True); call(); prof, _ = api.profile_read(); api.profile_enable(False)
        api.profile_enable(True); api.demux_locate(dev, tags, window=args.window, max_ed=args.max_ed); prof_l, _ = api.profile_read(); api.profile_enable(False)
        per_read = np.diff(hit_off.astype(np.int64))
        launches, scan_ms = prof["k_demux_scan"][0], prof["k_demux_scan"][1]
        scan_cols = len(patterns) * bases * launches                       # lane-columns of all launches of the profiled call
        loc_cols = n * 2 * len(tags) * args.window
        line = dict(config=cfg, mode="scan", reads=n, concatemers=n_conc, patterns=len(patterns), bases=bases, hits=int(len(hits)), reads_with_more_than_two_hits=int((per_read > 2).sum()),
                    demux_scan_ms=round(float(np.median(ts)) * 1e3, 2), demux_scan_runs_ms=[round(x * 1e3, 2) for x in ts],
                    k_demux_scan_ms=round(scan_ms, 3), k_demux_scan_launches=launches, k_demux_scan_ms_per_launch=round(scan_ms / launches, 3),
                    k_demux_locate_ms=round(prof_l["k_demux_locate"][1], 3),
                    scan_lane_columns_per_s=round(scan_cols / (scan_ms / 1e3)), locate_lane_columns_per_s=round(loc_cols / (prof_l["k_demux_locate"][1] / 1e3)))
        line["scan_over_locate_rate"] = round(line["scan_lane_columns_per_s"] / line["locate_lane_columns_per_s"], 3)
        m = min(args.scan_host_reads, n)
        off = rs.off.astype(np.int64)
        sub = [rs.seq[off[i]:off[i + 1]].tobytes().decode() for i in range(m)]
        t0 = time.perf_counter(); want = sref.scan(sub, patterns, args.max_ed); sec = time.perf_counter() - t0
        assert np.array_equal(want[1], hits[:int(hit_off[m])]) and np.array_equal(want[0], hit_off[:m + 1])
        line["numpy_reference_ms"] = round(sec / m * n * 1e3, 1)
        line["numpy_reference_note"] = "extrapolated: %d reads in %.2f s on one thread (equal to the device's hits), scaled to %d reads, not run" % (m, sec, n)
        print(json.dumps(line), flush=True)
        dev.release()


def host_loop_seconds(lib, rs, tags, window, max_ed, sample_reads, threads=16):
    """seconds the 16-thread host loop takes for the first sample_reads reads, every (read end, tag) pair"""
    from concurrent.futures import ThreadPoolExecutor
    fn = lib.ngsid_host_infix_locate
    tg = [t.encode() for t in tags]
    off = rs.off.astype(np.int64)
    wins = []
    for i in range(sample_reads):
        a = rs.seq[off[i]:off[i + 1]]; w = min(window, len(a))
        wins.append(a[:w].tobytes()); wins.append(COMP[a[::-1][:w]].tobytes())

    def work(part):
        ed, st, en = C.c_int32(), C.c_int32(), C.c_int32()
        for w in part:
            for q in tg:
                fn(q, C.c_int32(len(q)), w, C.c_int32(len(w)), C.c_int32(max_ed), C.c_int32(1), C.byref(ed), C.byref(st), C.byref(en))
    parts = [wins[k::threads] for k in range(threads)]
    with ThreadPoolExecutor(max_workers=threads) as ex:
        t0 = time.perf_counter(); list(ex.map(work, parts)); return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="100000x24,1000000x96", help="reads x dual tags")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=int, default=150); ap.add_argument("--max_ed", type=int, default=3)
    ap.add_argument("--host_sample", type=int, default=0, help="reads of the first configuration the host loop is timed on (0 = all of them)")
    ap.add_argument("--scan", action="store_true", help="measure ngsid_demux_scan (and k_demux_locate on the same reads) instead")
    ap.add_argument("--scan_host_reads", type=int, default=4, help="--scan: reads the numpy reference is timed on")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from ngspeciesid_amd import runtime
    api = runtime.get_api(0)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), window=args.window, max_ed=args.max_ed, repeats=args.repeats)), flush=True)
    if args.scan:
        return scan_bench(api, args)
    host_rate = None
    for cfg in args.configs.split(","):
        n, d = (int(x) for x in cfg.split("x"))
        rs, tags = make_pool(n, d, seed=1000 + d)
        dev = api.upload_reads(rs)
        call = lambda: api.demux_locate(dev, tags, window=args.window, max_ed=args.max_ed)
        hits = call()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter(); call(); ts.append(time.perf_counter() - t0)
        api.profile_enable(True); call(); prof, _ = api.profile_read(); api.profile_enable(False)
        pairs = n * 2 * len(tags)
        line = dict(config=cfg, reads=n, tags=len(tags), pairs=pairs, found_both_ends=round(float((hits[:, :, 0] >= 0).all(axis=1).mean()), 4),
                    demux_locate_ms=round(float(np.median(ts)) * 1e3, 2), demux_locate_runs_ms=[round(x * 1e3, 2) for x in ts],
                    k_demux_locate_ms=round(prof["k_demux_locate"][1], 3), k_demux_locate_launches=prof["k_demux_locate"][0])
        line["pairs_per_s_kernel"] = round(pairs / (line["k_demux_locate_ms"] / 1e3))
        if host_rate is None:
            m = n if args.host_sample <= 0 else min(args.host_sample, n)
            sec = host_loop_seconds(api.lib, rs, tags, args.window, args.max_ed, m)
            host_rate = m * 2 * len(tags) / sec
            line["host_16_threads_ms"] = round(pairs / host_rate * 1e3, 1)
            line["host_16_threads_note"] = "measured: one run over all pairs" if m == n else "measured on the first %d reads (%.2f s), scaled to %d reads" % (m, sec, n)
        else:
            line["host_16_threads_ms"] = round(pairs / host_rate * 1e3, 1)
            line["host_16_threads_note"] = "extrapolated from the pair rate of the first configuration, not run"
        line["host_over_device_call"] = round(line["host_16_threads_ms"] / line["demux_locate_ms"], 1)
        print(json.dumps(line), flush=True)
        dev.release()


if __name__ == "__main__":
    main()
