"""What a minimum-edit alignment does to a KNOWN error model, on the CPU, with the reference definition of the device call (tests/errprof_reference.py on the oracle) - no GPU.

Sets: synth.make_reads (C3's read profile: 5 species of 750 bases at 15 % divergence, both strands) at mu = 17 and mu = 14, --reads (1 000) reads a set, --seeds (5) seeds,
every read listed under the amplicon that generated it - NOT under a consensus made of the reads, so nothing here is hidden by a shared error.  The generator makes a base
an error with probability 10^(-q / 10) of its own quality q and splits the errors 40 / 30 / 30 into substitutions, deletions and insertions; an inserted base carries the
quality of the base it follows, a deleted base leaves no quality behind.  So of the errors a READ base can show (mismatch or insertion) the generator implies
0.7 * 10^(-q / 10) per base of quality q: a calibration line 1.55 above the diagonal.

The tool RECORDS how far the recovered figures are from the generator's: errors that cancel (an insertion next to a deletion is one mismatch), a substituted base that
equals its neighbour and slides into a gap, and indels that the aligner's tie-break places inside a homopolymer.  No test asserts a tolerance on any of it.

    python tools/errprof_sweep.py [--seeds 5] [--reads 1000] >> profiles/errprof.txt"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def one_set(oracle, mu, seed, n_reads):
    from ngspeciesid_amd import synth
    from ngspeciesid_amd._capi import ReadSet
    from errprof_reference import errprof_reference
    sp = synth.make_species(5, 750, 0.15, seed=seed + 1)
    rd = synth.make_reads(sp, n_reads, mu=mu, seed=100 + seed, rc_fraction=0.5)
    rs = ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64)); species = rd["species"].numpy()
    lists = [np.nonzero(species == g)[0].astype(np.uint32) for g in range(len(sp))]
    grp = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
    counts, qtab, strand = errprof_reference(oracle, [s.tobytes().decode() for s in sp], rs, grp, np.concatenate(lists))
    q = rd["qual"].numpy().astype(np.float64) - 33.0
    return counts.sum(axis=0), qtab.sum(axis=0), int((strand >= 0).sum()), float((10.0 ** (-q / 10.0)).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=5); ap.add_argument("--reads", type=int, default=1000)
    args = ap.parse_args()
    from oracle_lib import load_oracle
    from ngspeciesid_amd import errprof
    oracle = load_oracle()
    print("# tools/errprof_sweep.py: the CPU reference on synth.make_reads against the GENERATING amplicons, %d seeds x %d reads per mu.  One JSON line per mu." % (args.seeds, args.reads))
    print("# generator: errors 40 / 30 / 30 substitution / deletion / insertion, drawn with probability 10^(-q / 10); a read base of quality q shows 0.7 of it (implied_q = q + 1.55)")
    for mu in (17.0, 14.0):
        counts = 0; qtab = 0; used = 0; gen = []
        for seed in range(args.seeds):
            c, q, u, p = one_set(oracle, mu, seed, args.reads)
            counts = counts + c; qtab = qtab + q; used += u; gen.append(p)
        r = errprof.rates(counts)["both"]; su = errprof.summary(counts, qtab); cal = errprof.calibration(qtab, min_obs=1000); il = errprof.indel_lengths(counts); hp = errprof.hp_table(counts)
        tot = r["total"]
        line = dict(mu=mu, seeds=args.seeds, reads=args.seeds * args.reads, reads_with_a_strand=used, generator_error_per_base=round(float(np.mean(gen)), 5),
                    recovered_rates={k: round(v, 5) for k, v in r.items()},
                    recovered_split_sub_ins_del=[round(r["substitution"] / tot, 4), round(r["insertion"] / tot, 4), round(r["deletion"] / tot, 4)], generator_split_sub_ins_del=[0.4, 0.3, 0.3],
                    read_error_rate=round(su["error_rate"], 5), read_error_phred=round(su["phred"], 2), reported_error=round(su["reported_error"], 5), reported_phred=round(su["reported_phred"], 2),
                    ins_runs_of_1_2_3plus=[round(float(il["ins_share"][0]), 4), round(float(il["ins_share"][1]), 4), round(float(il["ins_share"][2:].sum()), 4)],
                    del_runs_of_1_2_3plus=[round(float(il["del_share"][0]), 4), round(float(il["del_share"][1]), 4), round(float(il["del_share"][2:].sum()), 4)],
                    hp_run_1_2_3_4plus_sub_del_ins=[[round(float(hp[k][i] if i < 3 else (hp[k][3:] * hp["n"][3:]).sum() / max(1, hp["n"][3:].sum())), 5) for k in ("sub", "dele", "ins_behind")] for i in range(4)],
                    calibration=[dict(q=int(q_), n=int(a + b + c_), empirical_q=round(float(e), 2), implied_q=round(q_ + 1.549, 2), diagonal=int(q_))
                                 for q_, a, b, c_, e in zip(cal["q"], cal["n_match"], cal["n_sub"], cal["n_ins"], cal["empirical_q"]) if q_ % 5 == 0 or q_ in (1, 50)])
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
