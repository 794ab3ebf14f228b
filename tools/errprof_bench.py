"""ngsid_error_profile on one GPU, beside the other consumers of the store pass on the same reads in the same process: what the fifth consumer costs, with and without qtab.

Shape: that of tools/cigar_bench.py - --reads (10^6) synthetic reads of 5 amplicons of 750 bases at mu = 14, every read listed under its own amplicon.

    python tools/errprof_bench.py [--reads 1000000] [--repeats 3] [--out FILE]

One JSON line: the wall time of Api.error_profile with and without qtab, of Api.consensus_support, Api.hp_runs and Api.read_cigars with a known cap (host clock around the
call; median of --repeats runs after one warm-up); the HIP-event time per kernel of one profiled run of each; k_errprof over k_ed_align_rec of the same call - the
yardstick: a reader of the path matrix should not take longer than the DP that wrote it -; the bytes k_errprof reads per second (span, nibbles, read positions, centre
bytes and, with qtab, the qualities) against the 8 TB/s HBM peak the roofline lines of this project use; and the rates the profile finds, beside the generator's."""
import argparse, json, os, sys, time
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
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from ngspeciesid_amd import runtime, synth, hp, errprof
    from ngspeciesid_amd._capi import ReadSet, ERRPROF_PAIR
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
    needed = len(api.read_cigars(cen, rs, grp, read_order=ro)[2])
    calls = dict(error_profile=lambda: api.error_profile(cen, rs, grp, read_order=ro),
                 error_profile_no_qtab=lambda: api.error_profile(cen, rs, grp, read_order=ro, qualities=False),
                 consensus_support=lambda: api.consensus_support(cen, rs, grp, read_order=ro),
                 hp_runs=lambda: api.hp_runs(cen, rs, grp, run_off, run_start, read_order=ro),
                 read_cigars_fill_only=lambda: api.read_cigars(cen, rs, grp, read_order=ro, cap=needed))
    line = dict(device=torch.cuda.get_device_name(0), reads=int(grp[-1]), length=args.length, centres=args.species, mu=args.mu, repeats=args.repeats)
    res = {}
    for name in calls:
        res[name], line[name + "_ms"], line[name + "_runs_ms"] = timed(calls[name], args.repeats)
    counts, qtab, strand = res["error_profile"]
    assert np.array_equal(counts, res["error_profile_no_qtab"][0]) and res["error_profile_no_qtab"][1] is None
    line["strands_equal_hp_runs"] = bool(np.array_equal(strand, res["hp_runs"][1]))
    kern = {}
    for name in calls:
        api.profile_enable(True); api.profile_read(); calls[name](); prof, _ = api.profile_read(); api.profile_enable(False)
        kern[name] = {k_: [int(v_[0]), round(v_[1], 3)] for k_, v_ in prof.items() if k_.startswith(("k_", "host_"))}
    line["kernels_launches_ms"] = kern
    for name in ("error_profile", "error_profile_no_qtab"):
        k = kern[name]
        if "k_errprof" in k and k.get("k_ed_align_rec", [0, 0])[1] > 0:
            line["k_errprof_over_k_ed_align_rec" + name[len("error_profile"):]] = round(k["k_errprof"][1] / k["k_ed_align_rec"][1], 4)
    # bytes the kernel reads: per pair the span (16), per counted position the nibble (0.5), the read position (2), the centre byte (1) and, with qtab, the quality (1)
    cols = int(counts[:, :, ERRPROF_PAIR:ERRPROF_PAIR + 24].sum()); reads_used = int(counts[:, :, 30].sum())
    for name, per in (("error_profile", 4.5), ("error_profile_no_qtab", 2.5)):
        ms = kern[name].get("k_errprof", [0, 0])[1]
        if ms > 0:
            b = 16 * reads_used + per * cols; sfx = name[len("error_profile"):]
            line["k_errprof_read_bytes" + sfx] = int(b); line["k_errprof_read_GBps" + sfx] = round(b / (ms * 1e-3) / 1e9, 1); line["k_errprof_fraction_of_hbm_peak" + sfx] = round(b / (ms * 1e-3) / HBM_PEAK, 4)
    r = errprof.rates(counts)["both"]; su = errprof.summary(counts, qtab)
    line["rates"] = {k_: round(v_, 6) for k_, v_ in r.items()}
    tot = r["total"] or 1.0
    line["split_sub_ins_del"] = [round(r["substitution"] / tot, 4), round(r["insertion"] / tot, 4), round(r["deletion"] / tot, 4)]; line["generator_split"] = [0.4, 0.3, 0.3]
    line["summary"] = {k_: (round(v_, 6) if isinstance(v_, float) else v_) for k_, v_ in su.items()}
    s = json.dumps(line); print(s, flush=True)
    if args.out:
        with open(args.out, "a") as fh: fh.write(s + "\n")


if __name__ == "__main__":
    main()
