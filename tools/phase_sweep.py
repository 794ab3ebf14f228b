"""Settles the policy defaults of ngspeciesid_amd/phase.py on the CPU, with the reference definition of the device calls (tests/phase_reference.py on the oracle) - no GPU.

True splits: two haplotypes of a 700-base amplicon x {1, 3, 8} SNPs, with and without a 1-base indel difference, pooled 50/50 and 80/20, mu = 17 and 14, 300 reads.
False splits: ONE template whose amplicon holds homopolymers of 5 - 8 bases, mu = 14, 300 reads, --false_seeds seeds (the deletions of a run are all placed at one
of its columns by the aligner: 10 - 20 % `del` at that column, independent between columns).
Per case: the candidate sites, the kept sites, the haplotypes found, the share of reads the margin rule leaves out, the share of placed reads that went to the wrong
haplotype.  Usage: python tools/phase_sweep.py [--false_seeds 20] [--set name=value ...] > profiles/phase.txt"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from oracle_lib import load_oracle
from phase_reference import PhaseAdapter
import phase_cases as pc
from ngspeciesid_amd import phase, synth

L = 700
SNPS = {1: (350,), 3: (100, 350, 600), 8: (60, 130, 210, 300, 390, 470, 560, 640)}
RUNS = ((80, 5), (190, 6), (310, 7), (430, 8), (520, 6), (610, 8))


def run_case(api, templates, n_each, mu, seed, policy):
    rs, origin = pc.pooled(templates, n_each, mu, seed)
    e = phase.split(api, rs, templates[0], np.arange(rs.n, dtype=np.uint32), **policy)
    return e, origin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--false_seeds", type=int, default=20)
    ap.add_argument("--true_seeds", type=int, default=2)
    ap.add_argument("--set", nargs="*", default=[])
    a = ap.parse_args()
    policy = {}
    for kv in a.set:
        k, v = kv.split("="); policy[k] = type(phase.DEFAULTS[k])(float(v))
    api = PhaseAdapter(load_oracle())
    print("policy: %s" % dict(phase.DEFAULTS, **policy))
    base = synth.make_species(1, L, 0.0, indel=0.0, seed=11)[0].tobytes().decode()
    print("# true splits: snps indel mix mu seed -> kept sites, haplotypes (reads), excluded share, misplaced share of the placed reads")
    bad = 0
    for nsnp, snps in SNPS.items():
        for indel in (None, 250):
            for mix in ((150, 150), (240, 60)):
                for mu in (17.0, 14.0):
                    for seed in range(a.true_seeds):
                        t2 = pc.variant(base, snps, indel)
                        e, origin = run_case(api, [base, t2], list(mix), mu, 1000 + 37 * seed + nsnp, policy)
                        if e is None:
                            print("%d %s %d/%d %.0f %d -> NO SPLIT" % (nsnp, "indel" if indel else "-", mix[0], mix[1], mu, seed)); bad += 1; continue
                        asg = e["assign"]; placed = asg >= 0
                        # a haplotype's template = the one most of its reads came from
                        tmpl = [int(np.bincount(origin[asg == h], minlength=2).argmax()) for h in range(len(e["alleles"]))]
                        wrong = sum(int((origin[asg == h] != tmpl[h]).sum()) for h in range(len(tmpl)))
                        ok = len(tmpl) == 2 and sorted(tmpl) == [0, 1]
                        bad += not ok
                        print("%d %s %d/%d %.0f %d -> sites %s haps %s excluded %.3f misplaced %.4f%s" % (nsnp, "indel" if indel else "-", mix[0], mix[1], mu, seed, (e["sites"] + 1).tolist(),
                              ["%s:%d" % (phase.allele_string(r), n) for r, n in zip(e["alleles"], e["n_reads"])], 1.0 - placed.mean(), wrong / max(int(placed.sum()), 1), "" if ok else "  <-- NOT the two templates"))
    print("true splits that failed: %d" % bad)
    print("# false splits: one template with homopolymers %s (position, length), mu 14, 300 reads" % (RUNS,))
    hp = pc.with_homopolymers(base, RUNS); false = 0
    for seed in range(a.false_seeds):
        rs, _ = pc.pooled([hp], 300, 14.0, 5000 + seed)
        counts = api.consensus_support(pc.ReadSet.from_strings([hp]), rs, [0, rs.n])[0]
        cand = phase.candidate_sites(counts, hp, **{k: v for k, v in dict(phase.DEFAULTS, **policy).items() if k in ("min_alt_frac", "min_alt_reads")})
        e = phase.split(api, rs, hp, np.arange(rs.n, dtype=np.uint32), support=counts, **policy)
        false += e is not None
        print("seed %d: candidates %s -> %s" % (seed, (cand + 1).tolist(), "None" if e is None else "SPLIT at %s" % (e["sites"] + 1).tolist()))
    print("false splits: %d of %d" % (false, a.false_seeds))


if __name__ == "__main__":
    main()
