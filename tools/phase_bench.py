"""ngsid_phase_genotypes / ngsid_phase_pair_tables / ngsid_phase_assign on one GPU, beside ngsid_consensus_support on the same reads in the same process.

Shape: the final centres of the C3 workload - --reads (10^6) synthetic reads of 5 amplicons of 750 bases, every read listed under its own amplicon - with 64 evenly
spaced sites per centre and 4 haplotypes per centre (random allele strings with a fifth of the entries wild).

    python tools/phase_bench.py [--reads 1000000] [--repeats 3] [--out FILE]

One JSON line: the wall time of every call (host clock around the call, which ends in a stream synchronise; median of --repeats runs after one warm-up), the HIP-event
time per kernel of one profiled run of each, the ratios to the support call, and the size of the genotype matrix that crosses the boundary."""
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
    ap.add_argument("--sites", type=int, default=64); ap.add_argument("--haps", type=int, default=4); ap.add_argument("--mu", type=float, default=14.0)
    ap.add_argument("--repeats", type=int, default=3); ap.add_argument("--out", default=None, help="the JSON line is appended to this file")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from ngspeciesid_amd import runtime, synth
    from ngspeciesid_amd._capi import ReadSet
    api = runtime.get_api(0)
    sp = synth.make_species(args.species, args.length, 0.15, seed=3)
    rd = synth.make_reads(sp, args.reads, mu=args.mu, seed=4, device="cuda", rc_fraction=0.5)
    rs = ReadSet.from_torch(rd["seq"], rd["qual"], rd["off"])
    species = rd["species"].cpu().numpy()
    lists = [np.nonzero(species == g)[0].astype(np.uint32) for g in range(args.species)]
    grp = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64); ro = np.concatenate(lists)
    centres = [s.tobytes().decode() for s in sp]; cen = ReadSet.from_strings(centres)
    sites = [np.unique(np.linspace(0, len(c) - 1, args.sites).astype(np.int64)).astype(np.uint32) for c in centres]
    site_off = np.concatenate(([0], np.cumsum([len(s) for s in sites]))).astype(np.uint64); site_pos = np.concatenate(sites)
    rng = np.random.default_rng(5)
    hap_off = (np.arange(args.species + 1) * args.haps).astype(np.uint64)
    hal = np.concatenate([np.where(rng.random((args.haps, len(s))) < 0.2, 255, rng.integers(0, 5, (args.haps, len(s)))).astype(np.uint8).ravel() for s in sites])

    calls = dict(
        consensus_support=lambda: api.consensus_support(cen, rs, grp, read_order=ro),
        phase_genotypes=lambda: api.phase_genotypes(cen, rs, grp, site_off, site_pos, read_order=ro))
    line = dict(device=torch.cuda.get_device_name(0), reads=int(grp[-1]), length=args.length, centres=args.species, sites_per_centre=args.sites, haplotypes_per_centre=args.haps,
                mu=args.mu, repeats=args.repeats)
    res = {}
    for name in ("consensus_support", "phase_genotypes"):
        res[name], line[name + "_ms"], line[name + "_runs_ms"] = timed(calls[name], args.repeats)
    geno = res["phase_genotypes"][0]
    calls["phase_pair_tables"] = lambda: api.phase_pair_tables(geno, grp, site_off)
    calls["phase_assign"] = lambda: api.phase_assign(geno, grp, site_off, hap_off, hal)
    for name in ("phase_pair_tables", "phase_assign"):
        res[name], line[name + "_ms"], line[name + "_runs_ms"] = timed(calls[name], args.repeats)
    line["geno_bytes"] = int(len(geno)); line["pair_table_increments"] = int(res["phase_pair_tables"][0].sum())
    line["strand_called"] = round(float((res["phase_genotypes"][2] >= 0).mean()), 4); line["assigned"] = round(float((res["phase_assign"][0] >= 0).mean()), 4)
    # the invariant of the definition, on the whole matrix: per site the codes <= 5 are the support's depth
    sup = res["consensus_support"][0]; cen_off = res["consensus_support"][1]; goff = res["phase_genotypes"][1]; ok = True
    for g in range(args.species):
        m = geno[int(goff[g]):int(goff[g + 1])].reshape(len(lists[g]), len(sites[g]))
        ok = ok and bool(np.array_equal((m <= 5).sum(axis=0), sup[int(cen_off[g]) + sites[g].astype(np.int64), 0]))
    line["depth_equals_support"] = ok
    kern = {}
    for name in calls:
        api.profile_enable(True); calls[name](); prof, _ = api.profile_read(); api.profile_enable(False)
        kern[name] = {k_: [int(v_[0]), round(v_[1], 3)] for k_, v_ in prof.items() if k_.startswith(("k_", "host_"))}
    line["kernels_launches_ms"] = kern
    for name in ("phase_genotypes", "phase_pair_tables", "phase_assign"):
        line[name + "_over_support"] = round(line[name + "_ms"] / line["consensus_support_ms"], 3)
    s = json.dumps(line); print(s, flush=True)
    if args.out:
        with open(args.out, "a") as fh: fh.write(s + "\n")


if __name__ == "__main__":
    main()
