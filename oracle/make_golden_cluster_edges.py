#!/usr/bin/env python3
"""Build container only: tests/golden/cluster_edges.npz = the read sets of tests/cluster_cases.py and, for every call of every case, the verdict of the REFERENCE'S OWN
cluster.reads_to_clusters (imported and run like oracle/make_golden.py does: parasail is oracle/ref_shim, get_best_cluster / get_best_cluster_block_align are traced).

Calls with prev_batch / known_err hand the reference what parallelize.py hands it in a merge round: 8-tuples (id, batch, acc, seq, qual, score, error rate, HPC sequence) for
the reads whose error rate is known, 6-tuples for the others, and the minimizer database of the lower-batch representatives.  A KeyError of the p-table lookup
(cluster.py:367) is recorded as the expected error.  The derived calls of case (d) sit at the mapping / alignment ratios this script reads from the reference's trace.
Only data goes into the fixture.      make -C oracle && python oracle/make_golden_cluster_edges.py      (re-executes itself with PYTHONHASHSEED=0)"""
import os, sys
if os.environ.get("PYTHONHASHSEED") != "0":
    os.environ["PYTHONHASHSEED"] = "0"
    os.execv(sys.executable, [sys.executable] + sys.argv)
import itertools
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import make_golden as G                                   # the harness: shim + reference on sys.path, ref_args, p_table, csr
import parasail                                           # the shim (its CALLS log counts the aligner pairs)
from modules import cluster                               # the reference
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cluster_cases as CC
from oracle_lib import load_oracle

ST_NEWREP, ST_MAPPED, ST_ALIGNED, ST_SHORT, ST_SEEDED = 0, 1, 2, 3, 4


def hpc(s):
    return "".join(ch for ch, _ in itertools.groupby(s))


def run_reference(case, call):
    """one call of reads_to_clusters -> dict of per-read arrays; 'aln_ratio' is what get_best_cluster_block_align returned as its ratio (case (d) reads it)"""
    n, k, w = len(case.seqs), case.k, case.w
    args = G.ref_args(k=k, w=w, nr_cores=1, min_shared=int(call.prm["min_shared"]), min_fraction=call.prm["min_fraction"], mapped_threshold=call.prm["mapped_threshold"],
                      aligned_threshold=call.prm["aligned_threshold"], min_prob_no_hits=call.prm["min_prob_no_hits"], symmetric_map_align_thresholds=bool(call.prm["symmetric"]))
    if call.ptab == "select": pt = G.p_table(k, w)
    else:
        t = CC.round2_table(call.known_err[1], call.known_err[0]).reshape(15, 15)
        pt = {((i + 1) / 100.0, (j + 1) / 100.0): float(t[i, j]) for i in range(15) for j in range(15) if not np.isnan(t[i, j])}
    prev = call.prev_batch if call.prev_batch is not None else np.zeros(n, dtype=np.int32)
    lowest = max(1, int(prev.min())) if call.prev_batch is not None else 1
    read_array = [(i, int(prev[i]), case.acc[i], case.seqs[i], case.quals[i], float(n - i)) for i in range(n)]
    clusters, representatives, db = {}, {}, {}
    for i, b, acc, seq, qual, score in read_array:
        clusters[i] = [acc]
        known = call.known_err is not None and not np.isnan(call.known_err[i])
        representatives[i] = (i, b, acc, seq, qual, score, float(call.known_err[i]), hpc(seq)) if known else (i, b, acc, seq, qual, score)
        if call.prev_batch is not None and b == lowest:      # a representative of the lower batch: its minimizers are the database handed over (parallelize.py:209-215)
            assert known, "a seeded read carries its error rate"
            if len(hpc(seq)) >= k:
                for m, _ in cluster.get_kmer_minimizers(hpc(seq), k, w): db.setdefault(m, set()).add(i)
    trace, aln, pairs = {}, {}, np.zeros(n, dtype=np.int32)
    orig_gbc, orig_gba = cluster.get_best_cluster, cluster.get_best_cluster_block_align

    def gbc(read_cl_id, *a, **kw):
        r = orig_gbc(read_cl_id, *a, **kw); trace[read_cl_id] = r; return r

    def gba(read_cl_id, *a, **kw):
        before = len(parasail.CALLS)
        r = orig_gba(read_cl_id, *a, **kw)
        pairs[read_cl_id] = len(parasail.CALLS) - before; aln[read_cl_id] = (r[0], r[5]); return r
    cluster.get_best_cluster, cluster.get_best_cluster_block_align = gbc, gba
    error = 0
    try:
        res = cluster.reads_to_clusters(clusters, representatives, read_array, pt, db, 1, args)
        clusters, representatives, _, _ = list(res.values())[0]
    except KeyError:
        error = 1
    finally:
        cluster.get_best_cluster, cluster.get_best_cluster_block_align = orig_gbc, orig_gba
    out = dict(rep_of=np.arange(n, dtype=np.int32), status=np.zeros(n, dtype=np.uint8), tr_best=np.full(n, -2, dtype=np.int32), tr_ns=np.zeros(n, dtype=np.int32),
               tr_ratio=np.zeros(n), counters=np.zeros(3, dtype=np.int64), pairs=pairs, error=np.int32(error), aln_ratio=np.full(n, np.nan))
    if error: return out
    acc2i = {a: i for i, a in enumerate(case.acc)}
    for cid, accs in clusters.items():
        for a in accs: out["rep_of"][acc2i[a]] = cid
    for i in range(n):
        if call.prev_batch is not None and prev[i] == lowest: out["status"][i] = ST_SEEDED
        elif len(hpc(case.seqs[i])) < k: out["status"][i] = ST_SHORT
        elif trace[i][0] >= 0: out["status"][i] = ST_MAPPED
        elif i in aln and aln[i][0] >= 0: out["status"][i] = ST_ALIGNED
        else: out["status"][i] = ST_NEWREP
    for i, (b, s, r) in trace.items(): out["tr_best"][i], out["tr_ns"][i], out["tr_ratio"][i] = b, s, r
    for i, (b, r) in aln.items(): out["aln_ratio"][i] = r
    out["counters"][:] = [sum(1 for v in trace.values() if v[0] >= 0), sum(1 for v in aln.values() if v[0] >= 0), len(aln)]
    return out


def main():
    oracle = load_oracle()
    out = {"source": np.array("reads_to_clusters of the reference (NGSpeciesID v0.3.1), every case and call")}
    names = []
    for case in CC.all_cases(oracle):
        n = len(case.seqs)
        res = [run_reference(case, c) for c in case.calls]
        if case.name == "threshold_equalities":
            qm, qa = case.info["qm"], case.info["qa"]
            assert res[0]["status"][qm] == ST_MAPPED and res[1]["status"][qm] == ST_MAPPED and res[0]["status"][qa] == ST_ALIGNED and res[1]["status"][qa] == ST_ALIGNED
            case.calls += CC.threshold_calls(res[0]["tr_ratio"][qm], res[0]["aln_ratio"][qa], res[1]["tr_ratio"][qm], res[1]["aln_ratio"][qa])
            res += [run_reference(case, c) for c in case.calls[2:]]
        p = case.name + "__"
        out[p + "seq"], out[p + "off"] = G.csr(case.seqs); out[p + "qual"], _ = G.csr(case.quals)
        out[p + "acc"] = np.array(case.acc); out[p + "kw"] = np.array([case.k, case.w], dtype=np.int32)
        out[p + "tags"] = np.array([c.tag for c in case.calls])
        out[p + "prm"] = np.array([[float(c.prm[key]) for key in CC.PRM_KEYS] for c in case.calls])
        out[p + "ptab_round2"] = np.array([c.ptab == "round2" for c in case.calls])
        out[p + "has_prev"] = np.array([c.prev_batch is not None for c in case.calls]); out[p + "has_known"] = np.array([c.known_err is not None for c in case.calls])
        out[p + "prev"] = np.array([c.prev_batch if c.prev_batch is not None else np.zeros(n, dtype=np.int32) for c in case.calls], dtype=np.int32)
        out[p + "known"] = np.array([c.known_err if c.known_err is not None else np.full(n, np.nan) for c in case.calls])
        for key in ("rep_of", "status", "tr_best", "tr_ns", "tr_ratio", "counters", "pairs", "error"):
            out[p + key] = np.array([r[key] for r in res])
        names.append(case.name)
        print(case.name, n, "reads", len(case.calls), "calls; first call: new", int((res[0]["status"] == 0).sum()), "mapped/aligned/called", res[0]["counters"].tolist(),
              "max pairs", int(max(r["pairs"].max() for r in res)), "errors", int(sum(r["error"] for r in res)), flush=True)
    out["cases"] = np.array(names)
    path = os.path.join(G.GOLD, "cluster_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
