"""ngsid_hp_runs on one GPU, beside ngsid_consensus_support on the same reads in the same process: what the read positions of the store pass cost.

Shape: the final centres of the C3 workload - --reads (10^6) synthetic reads of 5 amplicons of 750 bases, every read listed under its own amplicon - with every run of
every centre listed (about 560 a centre).

    python tools/hp_bench.py [--reads 1000000] [--repeats 3] [--out FILE]

One JSON line: the wall time of both calls (host clock around the call, which ends in a stream synchronise; median of --repeats runs after one warm-up) and the HIP-event
time per kernel of one profiled run of each.  k_ed_align_rec of the hp_runs call writes the path AND the positions, the one of the support call the path only: that pair is
the price of the second output (the chunks of the hp call are a fifth as long under the same budget, so it also launches more often)."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    from ngspeciesid_amd import runtime, synth, hp
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
    calls = dict(consensus_support=lambda: api.consensus_support(cen, rs, grp, read_order=ro),
                 hp_runs=lambda: api.hp_runs(cen, rs, grp, run_off, run_start, read_order=ro))
    line = dict(device=torch.cuda.get_device_name(0), reads=int(grp[-1]), length=args.length, centres=args.species, runs=int(run_off[-1]), mu=args.mu, repeats=args.repeats)
    res = {}
    for name in calls:
        res[name], line[name + "_ms"], line[name + "_runs_ms"] = timed(calls[name], args.repeats)
    hist = res["hp_runs"][0]
    line["spanned_observations"] = int(hist.sum()); line["usable_share"] = round(float(hist[:, :, :16].sum()) / max(1, int(hist.sum())), 4)
    line["strands_equal_support"] = bool(np.array_equal(res["hp_runs"][1], res["consensus_support"][3]))
    kern = {}
    for name in calls:
        api.profile_enable(True); api.profile_read(); calls[name](); prof, _ = api.profile_read(); api.profile_enable(False)
        kern[name] = {k_: [int(v_[0]), round(v_[1], 3)] for k_, v_ in prof.items() if k_.startswith(("k_", "host_"))}
    line["kernels_launches_ms"] = kern
    line["hp_runs_over_support"] = round(line["hp_runs_ms"] / line["consensus_support_ms"], 3)
    a, b = kern["hp_runs"].get("k_ed_align_rec"), kern["consensus_support"].get("k_ed_align_rec")
    if a and b: line["k_ed_align_rec_with_positions_over_without"] = round(a[1] / b[1], 3)
    s = json.dumps(line); print(s, flush=True)
    if args.out:
        with open(args.out, "a") as fh: fh.write(s + "\n")


if __name__ == "__main__":
    main()
