"""What the recruit policy assigns, by min_margin, on synthetic families - CPU only: the hits come from the numpy restatement of ngsid_recruit
(tests/recruit_reference.py), the policy is ngspeciesid_amd/recruit.py.

Per configuration --species templates of --length letters from synth.make_species, every two of them about `apart` apart (each template carries apart / 2 substitutions
against the common root), and --reads reads of synth.make_reads on both strands at the read profile mu (17 = the C3 workload of bench.py, 14 = the noisy one).  The
templates themselves stand in for the final consensuses; the bound is recruit.thresholds at the default identity (0.80).  One JSON line per (apart, mu): the share
of reads with a hit, and per min_margin 1, 2 and 4 the share assigned, ambiguous and assigned to a template other than the read's own.  Reported numbers, not pass
criteria.

    python tools/recruit_sweep.py                  # apart 0.02, 0.05, 0.15 x mu 17, 14"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--apart", default="0.02,0.05,0.15"); ap.add_argument("--mu", default="17,14")
    ap.add_argument("--species", type=int, default=5); ap.add_argument("--length", type=int, default=600); ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--margins", default="1,2,4")
    args = ap.parse_args()
    import recruit_reference as ref
    from ngspeciesid_amd import recruit, synth
    for x, apart in enumerate(float(v) for v in args.apart.split(",")):
        sp = synth.make_species(args.species, args.length, apart / 2.0, seed=40 + x)
        cons = [s.tobytes().decode() for s in sp]
        for mu in (float(v) for v in args.mu.split(",")):
            rd = synth.make_reads(sp, args.reads, mu=mu, seed=50 + x, rc_fraction=0.5)
            seq = rd["seq"].numpy(); off = rd["off"].numpy(); truth = rd["species"].numpy()
            reads = [seq[off[i]:off[i + 1]].tobytes().decode() for i in range(args.reads)]
            hits = ref.recruit(reads, [0, len(reads)], cons, [0, len(cons)], recruit.thresholds([len(c) for c in cons]))
            line = dict(apart=apart, mu=mu, species=args.species, length=args.length, reads=args.reads, bound=int(recruit.thresholds([args.length])[0]),
                        with_a_hit=round(float((hits[:, 0] >= 0).mean()), 4), nearest_is_wrong=round(float(((hits[:, 0] >= 0) & (hits[:, 0] != truth)).mean()), 4),
                        strand_is_wrong=round(float(((hits[:, 0] >= 0) & (hits[:, 2] != rd["strand"].numpy())).mean()), 4))
            for mm in (int(v) for v in args.margins.split(",")):
                st = recruit.assign(hits, mm)
                got = st == recruit.ASSIGNED
                line["min_margin_%d" % mm] = dict(assigned=round(float(got.mean()), 4), ambiguous=round(float((st == recruit.AMBIGUOUS).mean()), 4),
                                                  assigned_to_the_wrong_template=round(float((got & (hits[:, 0] != truth)).mean()), 4))
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
