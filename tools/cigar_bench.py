"""ngsid_read_cigars on one GPU, beside ngsid_hp_runs on the same reads in the same process: what the fourth consumer of the store pass costs, and the SAM writer.

Shape: that of tools/hp_bench.py - --reads (10^6) synthetic reads of 5 amplicons of 750 bases, every read listed under its own amplicon.

    python tools/cigar_bench.py [--reads 1000000] [--repeats 3] [--out FILE]

One JSON line: the wall time of the count + fill call (cap=None), of the fill call alone with the known cap, and of Api.hp_runs (host clock around the call; median of
--repeats runs after one warm-up); the HIP-event time per kernel of one profiled run of each; ops per read; the bytes k_cigar_count / k_cigar_emit read per second (the
nibbles of every span and the 16 bytes of it, for the emit the two read positions of every insertion and the offsets as well; written ops beside) against the 8 TB/s
HBM peak the roofline lines of this project use; and the time ngsid_host_write_sam takes for the file of all reads (written to --tmp, removed again)."""
import argparse, json, os, sys, time, tempfile, shutil
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def timed(fn, repeats):
    out = fn(); ts = []
    for _ in range(repeats):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return out, round(float(np.median(ts)) * 1e3, 2), [round(t * 1e3, 2) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000); ap.add_argument("--length", type=int, default=750); ap.add_argument("--species", type=int, default=5)
    ap.add_argument("--mu", type=float, default=14.0); ap.add_argument("--repeats", type=int, default=3); ap.add_argument("--out", default=None, help="the JSON line is appended to this file")
    ap.add_argument("--tmp", default=None, help="folder for the SAM file (default: a temporary one)"); ap.add_argument("--no_sam", action="store_true")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from ngspeciesid_amd import runtime, synth, hp, sam, fastio
    from ngspeciesid_amd._capi import ReadSet
    api = runtime.get_api(0)
    sp = synth.make_species(args.species, args.length, 0.15, seed=3)
    rd = synth.make_reads(sp, args.reads, mu=args.mu, seed=4, device="cuda", rc_fraction=0.5)
    rs = ReadSet.from_torch(rd["seq"], rd["qual"], rd["off"])
    species = rd["species"].cpu().numpy()
    lists = [np.nonzero(species == g)[0].astype(np.uint32) for g in range(args.species)]
    grp = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64); ro = np.concatenate(lists)
    centres = [s.tobytes().decode() for s in sp]; cen = ReadSet.from_strings(centres)
    starts = [hp.runs(c)[0] for c in centres]
    run_off = np.concatenate(([0], np.cumsum([len(s) for s in starts]))).astype(np.uint64); run_start = np.concatenate(starts)
    first = api.read_cigars(cen, rs, grp, read_order=ro)
    needed = len(first[2])
    calls = dict(hp_runs=lambda: api.hp_runs(cen, rs, grp, run_off, run_start, read_order=ro),
                 read_cigars_count_and_fill=lambda: api.read_cigars(cen, rs, grp, read_order=ro),
                 read_cigars_fill_only=lambda: api.read_cigars(cen, rs, grp, read_order=ro, cap=needed))
    line = dict(device=torch.cuda.get_device_name(0), reads=int(grp[-1]), length=args.length, centres=args.species, mu=args.mu, repeats=args.repeats)
    res = {}
    for name in calls:
        res[name], line[name + "_ms"], line[name + "_runs_ms"] = timed(calls[name], args.repeats)
    aln, op_off, ops, strand = res["read_cigars_fill_only"]
    assert all(np.array_equal(x, y) for x, y in zip(res["read_cigars_fill_only"], res["read_cigars_count_and_fill"]))
    mapped = aln[:, 0] >= 0
    line["ops"] = int(needed); line["ops_per_read"] = round(needed / max(1, int(mapped.sum())), 2); line["mapped"] = int(mapped.sum())
    line["nm_per_read"] = round(float(aln[mapped, 4].mean()), 2); line["strands_equal_hp_runs"] = bool(np.array_equal(strand, res["hp_runs"][1]))
    kern = {}
    for name in calls:
        api.profile_enable(True); api.profile_read(); calls[name](); prof, _ = api.profile_read(); api.profile_enable(False)
        kern[name] = {k_: [int(v_[0]), round(v_[1], 3)] for k_, v_ in prof.items() if k_.startswith(("k_", "host_"))}
    line["kernels_launches_ms"] = kern
    line["fill_only_over_count_and_fill"] = round(line["read_cigars_fill_only_ms"] / line["read_cigars_count_and_fill_ms"], 3)
    line["fill_only_over_hp_runs"] = round(line["read_cigars_fill_only_ms"] / line["hp_runs_ms"], 3)
    # bytes the walk reads: per pair the span (16) and the nibbles of its positions; the emit also the offset and count (12) and two positions of 2 bytes per insertion
    span_pos = (aln[mapped, 1] - aln[mapped, 0] + 1).astype(np.int64).sum(); n_ins = int(((ops & 15) == 1).sum())
    k = kern["read_cigars_fill_only"]
    rd_count = 16 * int(mapped.sum()) + span_pos // 2; rd_emit = rd_count + 12 * int(mapped.sum()) + 4 * n_ins
    for nm, b in (("k_cigar_count", rd_count), ("k_cigar_emit", rd_emit)):
        if nm in k and k[nm][1] > 0:
            bps = b / (k[nm][1] * 1e-3)
            line[nm + "_read_bytes"] = int(b); line[nm + "_read_GBps"] = round(bps / 1e9, 1); line[nm + "_fraction_of_hbm_peak"] = round(bps / HBM_PEAK, 4)
    line["k_cigar_emit_written_bytes"] = int(4 * needed + 20 * int(mapped.sum()))
    if not args.no_sam:
        host = ReadSet(rd["seq"].cpu().numpy(), rd["qual"].cpu().numpy(), rd["off"].cpu().numpy().astype(np.uint64))
        names = fastio.Names.from_list(["read_%d" % i for i in range(host.n)])
        tmp = args.tmp or tempfile.mkdtemp(prefix="cigar_bench_")
        try:
            path = os.path.join(tmp, "reads_to_consensus.sam")
            tn = ["amplicon_%d" % g for g in range(args.species)]
            target = np.repeat(np.arange(args.species, dtype=np.int32), np.diff(grp.astype(np.int64)))
            head = sam.header(tn, [len(c) for c in centres])
            t0 = time.perf_counter()
            fastio.write_sam(path, head, ro, names, host, strand, target, tn, aln, op_off, ops)
            line["write_sam_ms"] = round((time.perf_counter() - t0) * 1e3, 1); line["sam_bytes"] = os.path.getsize(path)
            line["write_sam_GBps"] = round(line["sam_bytes"] / (line["write_sam_ms"] * 1e-3) / 1e9, 2)
        finally:
            if args.tmp is None: shutil.rmtree(tmp, ignore_errors=True)
            elif os.path.exists(os.path.join(tmp, "reads_to_consensus.sam")): os.remove(os.path.join(tmp, "reads_to_consensus.sam"))
    s = json.dumps(line); print(s, flush=True)
    if args.out:
        with open(args.out, "a") as fh: fh.write(s + "\n")


if __name__ == "__main__":
    main()
