"""ngsid_recruit on one GPU against the host locator in a 16-thread pool.

Seeded synthetic samples: per sample C consensuses of --cons_len letters (every second one a 10 % variant of the one before it, the others unrelated), reads of
--read_len letters = 50 random letters, a consensus with 4 % substitutions, random letters to the end; half of the reads reverse-complemented.  The bound per consensus
is recruit.thresholds at the default identity (0.80).

    python tools/recruit_bench.py                                 # 1x1000000x5, 1x1000000x30 and 96x10000x30 (samples x reads per sample x consensuses), both strands
    python tools/recruit_bench.py --configs 1x100000x5 --repeats 3

Per configuration one JSON line, with the plain instances and the cut-off instances of the kernel side by side on the same inputs (option "recruit_cutoff" 1 / 2; their
hit arrays are compared): the whole Api.recruit call (host clock around the call, which ends in a stream synchronise; median of --repeats runs after one warm-up;
device-resident reads), the k_recruit time of one profiled run (ngsid_profile_read: HIP events around the launches, summed), the word-columns per second of kernel
time (one word-column = one 64-row block of one pattern strand against one read letter, whether the kernel stepped it or not) and the block steps the waves took
(profiling line recruit_block_steps: one per wave, block and column) - block_steps_skipped_by_cut_off is one minus their ratio.
At the first configuration only, the comparator: ngsid_host_infix_locate over every (read, consensus strand) pair of the first --host_reads reads, called through ctypes
(which releases the interpreter lock) from 16 threads, one run, checked against the device's ed and end, and scaled to the configuration; for the other configurations
it is extrapolated from that word-column rate and labelled so."""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COMP = np.zeros(256, dtype=np.uint8)
for a, b in zip(b"ACGTN", b"TGCAN"):
    COMP[a] = b
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_samples(n_samples, per_sample, n_cons, cons_len, read_len, seed):
    """-> (ReadSet without qualities, read_off, consensuses as strings, cons_off)"""
    from ngspeciesid_amd._capi import ReadSet
    rng = np.random.default_rng(seed)
    cons = np.zeros((n_samples * n_cons, cons_len), dtype=np.uint8)
    for c in range(len(cons)):
        if c % n_cons and c % 2:
            cons[c] = cons[c - 1]
            pos = rng.random(cons_len) < 0.10
            cons[c, pos] = ACGT[rng.integers(0, 4, int(pos.sum()))]
        else:
            cons[c] = ACGT[rng.integers(0, 4, cons_len)]
    n = n_samples * per_sample
    seq = np.empty((n, read_len), dtype=np.uint8)
    lead = min(50, max(read_len - cons_len, 0)); body = min(cons_len, read_len - lead)
    for a in range(0, n, 100000):                                       # in blocks: the random draws of a million reads at once would take gigabytes
        b = min(n, a + 100000)
        blk = ACGT[rng.integers(0, 4, (b - a, read_len), dtype=np.uint8)]
        which = (np.arange(a, b) // per_sample) * n_cons + rng.integers(0, n_cons, b - a)
        src = cons[which][:, :body]
        noise = rng.integers(0, 256, src.shape, dtype=np.uint8) < 10    # 3.9 % of the letters redrawn
        src[noise] = ACGT[rng.integers(0, 4, int(noise.sum()), dtype=np.uint8)]
        blk[:, lead:lead + body] = src
        flip = rng.random(b - a) < 0.5
        blk[flip] = COMP[blk[flip][:, ::-1]]
        seq[a:b] = blk
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(read_len)
    return (ReadSet(seq.reshape(-1), None, off), np.arange(n_samples + 1, dtype=np.uint64) * np.uint64(per_sample),
            [c.tobytes().decode() for c in cons], np.arange(n_samples + 1, dtype=np.uint64) * np.uint64(n_cons))


def host_loop(lib, rs, read_off, cons, cons_off, bound, n_reads, threads=16):
    """the 16-thread host loop over every (read, consensus strand) pair of the first n_reads reads -> (seconds, word-columns, [(read, cons, strand, ed, end)])"""
    from concurrent.futures import ThreadPoolExecutor
    fn = lib.ngsid_host_infix_locate
    off = rs.off.astype(np.int64)
    group = np.searchsorted(np.asarray(read_off, dtype=np.int64), np.arange(n_reads), side="right") - 1
    strands = [(c.encode(), COMP[np.frombuffer(c.encode(), dtype=np.uint8)[::-1]].tobytes()) for c in cons]
    reads = [rs.seq[off[i]:off[i + 1]].tobytes() for i in range(n_reads)]
    wc = sum(len(reads[i]) * sum((len(cons[c]) + 63) // 64 for c in range(int(cons_off[group[i]]), int(cons_off[group[i] + 1]))) * 2 for i in range(n_reads))

    def work(part):
        ed, st, en = C.c_int32(), C.c_int32(), C.c_int32()
        out = []
        for i in part:
            x = reads[i]
            for c in range(int(cons_off[group[i]]), int(cons_off[group[i] + 1])):
                for s in (0, 1):
                    p = strands[c][s]
                    fn(p, C.c_int32(len(p)), x, C.c_int32(len(x)), C.c_int32(min(int(bound[c]), len(p) - 1)), C.c_int32(0), C.byref(ed), C.byref(st), C.byref(en))
                    out.append((i, c, s, ed.value, en.value))
        return out
    parts = [list(range(k, n_reads, threads)) for k in range(threads)]
    with ThreadPoolExecutor(max_workers=threads) as ex:
        t0 = time.perf_counter(); res = list(ex.map(work, parts)); sec = time.perf_counter() - t0
    return sec, wc, [r for part in res for r in part]


def check_against_host(hits, found, n_reads):
    """the device's best consensus of every read is the smallest (ed, index) of the host loop's hits, with its strand (a tie goes to forward) and end"""
    best = {}
    for i, c, s, ed, end in found:
        if ed >= 0 and (i not in best or (ed, c, s) < best[i][:3]):
            best[i] = (ed, c, s, end)
    for i in range(n_reads):
        want = best.get(i)
        got = hits[i].tolist()
        assert (got[0] < 0 and want is None) or (want is not None and (got[1], got[0], got[2], got[3]) == want), (i, got, want)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1x1000000x5,1x1000000x30,96x10000x30", help="samples x reads per sample x consensuses per sample")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cons_len", type=int, default=650); ap.add_argument("--read_len", type=int, default=750)
    ap.add_argument("--host_reads", type=int, default=2000, help="reads of the first configuration the host loop is timed on")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from ngspeciesid_amd import runtime, recruit
    api = runtime.get_api(0)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), cons_len=args.cons_len, read_len=args.read_len, repeats=args.repeats)), flush=True)
    host_rate = None
    for x, cfg in enumerate(args.configs.split(",")):
        ns, per, nc = (int(v) for v in cfg.split("x"))
        rs, read_off, cons, cons_off = make_samples(ns, per, nc, args.cons_len, args.read_len, seed=3000 + x)
        bound = recruit.thresholds([len(c) for c in cons])
        dev = api.upload_reads(rs)
        call = lambda: api.recruit(dev, read_off, cons, cons_off, bound)
        words = (args.cons_len + 63) // 64
        wc = rs.n * args.read_len * nc * 2 * words
        line = dict(config=cfg, samples=ns, reads=rs.n, consensuses_per_sample=nc, words_per_consensus=words, word_columns=wc)
        hits = None
        for family, key in ((1, "plain"), (2, "cut_off")):               # option "recruit_cutoff": the two kernel families on the same inputs
            api.set_option("recruit_cutoff", family)
            h = call()
            assert hits is None or np.array_equal(h, hits)
            hits = h
            ts = []
            for _ in range(args.repeats):
                t0 = time.perf_counter(); call(); ts.append(time.perf_counter() - t0)
            api.profile_enable(True); call(); prof, _ = api.profile_read(); api.profile_enable(False)
            steps = prof["recruit_block_steps"][0]
            line[key] = dict(recruit_ms=round(float(np.median(ts)) * 1e3, 1), recruit_runs_ms=[round(t * 1e3, 1) for t in ts],
                             k_recruit_ms=round(prof["k_recruit"][1], 2), k_recruit_launches=prof["k_recruit"][0],
                             word_columns_per_s_kernel=round(wc / (prof["k_recruit"][1] / 1e3)), wave_block_steps=steps)
        api.set_option("recruit_cutoff", 0)
        line["block_steps_skipped_by_cut_off"] = round(1.0 - line["cut_off"]["wave_block_steps"] / float(line["plain"]["wave_block_steps"]), 4)
        line["cut_off_over_plain_kernel_time"] = round(line["cut_off"]["k_recruit_ms"] / line["plain"]["k_recruit_ms"], 3)
        st = recruit.assign(hits)
        line.update(assigned=round(float((st == recruit.ASSIGNED).mean()), 4), ambiguous=round(float((st == recruit.AMBIGUOUS).mean()), 4))
        line["recruit_ms"] = min(line["plain"]["recruit_ms"], line["cut_off"]["recruit_ms"])
        if host_rate is None:
            m = min(args.host_reads, rs.n)
            sec, hwc, found = host_loop(api.lib, rs, read_off, cons, cons_off, bound, m)
            check_against_host(hits, found, m)
            host_rate = hwc / sec
            line["host_16_threads_note"] = "measured on the first %d reads (%d pairs, %.2f s, equal to the device's best hits), scaled to %d reads: extrapolated" % (m, len(found), sec, rs.n)
        else:
            line["host_16_threads_note"] = "extrapolated from the word-column rate of the first configuration, not run"
        line["host_16_threads_ms"] = round(wc / host_rate * 1e3, 1)
        line["host_over_device_call"] = round(line["host_16_threads_ms"] / line["recruit_ms"], 1)
        print(json.dumps(line), flush=True)
        dev.release()


if __name__ == "__main__":
    main()
