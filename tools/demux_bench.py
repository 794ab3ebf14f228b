"""ngsid_demux_locate on one GPU against the host locator in a 16-thread pool.

Seeded synthetic reads: a random 600-base amplicon body per read with a forward tag at the head and the reverse complement of a reverse tag at the tail (24-base
tags, 0 - 3 substitutions each, 0 - 30 random bases outside them; a fifth of the reads reverse-complemented).  "N dual tags" = N forward + N reverse tags, 2 N in all.

    python tools/demux_bench.py                                  # 100 k reads x 24 dual tags and 1 M reads x 96 dual tags; window 150, max_ed 3
    python tools/demux_bench.py --configs 100000x24 --repeats 5

Per configuration one JSON line: the whole demux_locate call (host clock around the call, which ends in a stream synchronise; median of --repeats runs after one
warm-up; device-resident reads) and the k_demux_locate time of one profiled run (ngsid_profile_read: HIP events around the launch).  At the first configuration
only, the comparator: ngsid_host_infix_locate over the same (read end, tag) pairs, called through ctypes (which releases the interpreter lock) from 16 threads, one
run (--host_sample N times it on the first N reads and scales); for the other configurations it is extrapolated from that pair rate and labelled so."""
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
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from ngspeciesid_amd import runtime
    api = runtime.get_api(0)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), window=args.window, max_ed=args.max_ed, repeats=args.repeats)), flush=True)
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
