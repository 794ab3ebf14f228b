#!/usr/bin/env python3
"""Settles the defaults of ngspeciesid_amd/chimera.py (min_gain, max_model_frac) on the CPU reference (tests/chimera_reference.py); no GPU.

Non-chimeric sets: families of 5-10 sequences of about 600 bases at 2 %, 5 % and 15 % pairwise divergence, every sequence with 0-2 residual errors (the quality of a
polished consensus); every sequence is modelled from ALL its siblings (any abundance order offers a subset of them).  Chimeric sets: the same families plus two-parent
chimeras with crossovers at 10 %, 50 % and 90 % of the length, modelled from the whole family.  Condition on the defaults: no sequence of the non-chimeric sets is
called.  Recall on the chimeras is recorded, not fixed in advance.  A setting is eligible only when max_model_frac x length admits MIN_MODEL_EDITS edits: a chimera's
consensus and its parents' carry residual errors of their own (up to 2 each here), and a threshold below that drops true chimeras for their polishing errors and
separates the real sequences of a 2 % family by a single edit.

    python tools/chimera_sweep.py [--sets 20] [--length 600] >> profiles/chimera.txt
"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import chimera_reference as ref
import chimera_cases as cases
from ngspeciesid_amd import chimera

GAINS = (1, 2, 3, 4, 5, 6, 8)
FRACS = (0.0025, 0.005, 0.0075, 0.01, 0.02, 0.03)
CROSS = (0.1, 0.5, 0.9)
MIN_MODEL_EDITS = 3


def residual(rng, s):
    """0-2 single-base errors"""
    for _ in range(int(rng.integers(0, 3))):
        i = int(rng.integers(0, len(s))); u = int(rng.integers(0, 3))
        c = cases.ALPHABET[int(rng.integers(0, 4))]
        s = s[:i] + (c + s[i + 1:] if u == 0 else c + s[i:] if u == 1 else s[i + 1:])
    return s


def model_all(queries, parents, skip_self):
    """every query against every parent (but itself, when the queries ARE the parents) -> fields"""
    pair_off, pair_parent = [0], []
    for q in range(len(queries)):
        pair_parent += [p for p in range(len(parents)) if not (skip_self and p == q)]
        pair_off.append(len(pair_parent))
    return ref.chimera_model(queries, parents, pair_off, pair_parent)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=20); ap.add_argument("--length", type=int, default=600); ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    t0 = time.time()
    rows = {}                                            # divergence -> (fields, lengths) of the real sequences; (divergence, crossover) -> the same of the chimeras
    minor = {}
    for div in (0.02, 0.05, 0.15):
        rng = np.random.default_rng(a.seed * 1000 + int(div * 100))
        for s in range(a.sets):
            fam = [residual(rng, x) for x in cases.family(rng, int(rng.integers(5, 11)), a.length, div)]
            f = model_all(fam, fam, True)
            rows.setdefault(div, []).append((f, [len(x) for x in fam]))
            for fr in CROSS:
                i, j = rng.permutation(len(fam))[:2]
                c, k = cases.chimera_of(fam[int(i)], fam[int(j)], fr)
                c = residual(rng, c)
                f = model_all([c], fam, False)
                rows.setdefault((div, fr), []).append((f, [len(c)]))
    print("# tools/chimera_sweep.py --sets %d --length %d --seed %d   (CPU reference, %.0f s)" % (a.sets, a.length, a.seed, time.time() - t0))
    for key, val in rows.items():
        f = np.concatenate([v[0] for v in val]); gain = f[:, 1] - f[:, 2]
        what = "real sequences, divergence %.2f" % key if not isinstance(key, tuple) else "chimeras, divergence %.2f, crossover %.1f" % key
        print("%-48s n=%4d  gain min/median/max %d/%d/%d   model_ed min/median/max %d/%d/%d" % (what, len(f), gain.min(), np.median(gain), gain.max(), f[:, 2].min(), np.median(f[:, 2]), f[:, 2].max()))
    print("min_gain max_model_frac  false_calls/real   recall by (divergence, crossover) ...")
    keys = [k for k in rows if isinstance(k, tuple)]
    print("%23s %18s   " % ("", "") + " ".join("%.2f/%.1f" % k for k in keys))
    clean = []                                           # (total recall, -min_gain, max_model_frac) of the settings without a false call
    for g in GAINS:
        for fr in FRACS:
            def called(key):
                f = np.concatenate([v[0] for v in rows[key]]); n = np.concatenate([v[1] for v in rows[key]])
                c = chimera.call(f, n, min_gain=g, max_model_frac=fr)
                return int(c.sum()), len(c)
            false = [called(k) for k in rows if not isinstance(k, tuple)]
            rec = [called(k) for k in keys]
            if sum(x[0] for x in false) == 0 and fr * a.length >= MIN_MODEL_EDITS: clean.append((sum(r[0] for r in rec), -g, fr))
            mark = "  <- defaults" if g == chimera.DEFAULTS["min_gain"] and fr == chimera.DEFAULTS["max_model_frac"] else ""
            print("%8d %14.3f  %6d/%-10d   " % (g, fr, sum(x[0] for x in false), sum(x[1] for x in false)) + " ".join("%3d/%-4d" % r for r in rec) + mark)
    best = max(clean)
    print("rule: among the settings without a false call that admit %d model edits, the highest total recall; then the smaller min_gain, then the larger max_model_frac -> min_gain %d, max_model_frac %g (recall %d/%d)"
          % (MIN_MODEL_EDITS, -best[1], best[2], best[0], sum(len(np.concatenate([v[1] for v in rows[k]])) for k in keys)))


if __name__ == "__main__":
    main()
