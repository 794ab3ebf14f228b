"""ngsid_refdb_build / ngsid_classify_search on one GPU against the numpy reference of the tests.

Seeded synthetic libraries: --base_species members come from synth.make_species (one root, 15 % substitutions, 1 % indels each: the members share conserved
stretches, so posting lists are long, as in COI); the rest of the library are copies of those members with 5 % substitutions drawn in numpy (make_species loops
over every base in Python: a million members would take longer than everything measured here).  A library of a million is therefore --base_species tight families of
about 500 members each: a query code hits on the order of a hundred references, far more than in a curated COI library - the posting lists are a worst case.  Queries: library members with 2 % substitutions, a third
reverse-complemented.

    python tools/classify_bench.py                               # 100 k x 650 and 1 M x 650 references; 200 and 2 000 queries each
    python tools/classify_bench.py --configs 100000x200 --out /tmp/classify.txt     # default: profiles/classify.txt

Per configuration one JSON line: library build time and sizes (ngsid_refdb_info), the whole classify_search call (host clock around the call, which ends in a
stream synchronise; median of --repeats runs after one warm-up), and the HIP-event time per kernel of one profiled run.  The
comparator is tests/classify_reference.py (Python sets over the library's own minimizer call), run ONCE at --ref_refs references x --ref_queries queries and
scaled by references x queries to the other sizes: every "reference_s" figure but that one is an extrapolation and is labelled so."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)
for a, b in zip(b"ACGT", b"TGCA"):
    COMP[a] = b


def substitute(rng, rows, rate):
    """rows [n, L] of ASCII ACGT with `rate` substitutions"""
    out = np.empty_like(rows)
    for a in range(0, len(rows), 65536):                                              # in slices: the random draws of a million rows at once would take 10 GB
        r = rows[a:a + 65536]
        hit = rng.random(r.shape, dtype=np.float32) < rate
        code = np.searchsorted(ACGT, r).astype(np.uint8)
        out[a:a + 65536] = np.where(hit, ACGT[(code + rng.integers(1, 4, r.shape, dtype=np.uint8)) % 4], r)
    return out


def make_library(n, length, base_species, seed):
    from ngspeciesid_amd import synth
    rng = np.random.default_rng(seed)
    nb = min(n, base_species)
    base = synth.make_species(nb, length + 16, 0.15, seed=seed)
    rows = np.stack([b[:length] for b in base])                                       # (indels shift a member by a few bases: cut to a common length)
    if n > nb:
        rows = np.concatenate([rows, substitute(rng, rows[rng.integers(0, nb, n - nb)], 0.05)])
    return rows


def make_queries(rows, nq, seed):
    rng = np.random.default_rng(seed + 1)
    member = rng.integers(0, len(rows), nq)
    q = substitute(rng, rows[member], 0.02)
    rc = np.arange(nq) % 3 == 2
    q[rc] = COMP[q[rc][:, ::-1]]
    return q, member, rc


def readset(rows):
    from ngspeciesid_amd._capi import ReadSet
    n, L = rows.shape
    return ReadSet(np.ascontiguousarray(rows).reshape(-1), None, np.arange(n + 1, dtype=np.uint64) * np.uint64(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="100000x200,100000x2000,1000000x200,1000000x2000", help="references x queries")
    ap.add_argument("--length", type=int, default=650); ap.add_argument("--base_species", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5); ap.add_argument("--top_k", type=int, default=8); ap.add_argument("--min_shared", type=int, default=3)
    ap.add_argument("--ref_refs", type=int, default=100000); ap.add_argument("--ref_queries", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classify.txt"), help="the JSON lines are also written to this file (replaced)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    import classify_reference as ref
    from ngspeciesid_amd import runtime
    api = runtime.get_api(0)
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True); lines.append(json.dumps(d))
    emit(dict(device=torch.cuda.get_device_name(0), length=args.length, k=13, w=20, top_k=args.top_k, min_shared=args.min_shared, repeats=args.repeats, base_species=args.base_species))
    ref_rate, libs = None, {}
    for cfg in args.configs.split(","):
        n, nq = (int(x) for x in cfg.split("x"))
        if n not in libs:
            libs.clear(); libs[n] = make_library(n, args.length, args.base_species, seed=2000)
        rows = libs[n]
        q, member, rc = make_queries(rows, nq, seed=n + nq)
        t0 = time.perf_counter(); db = api.refdb_build(readset(rows)); build_s = time.perf_counter() - t0
        dev = api.upload_reads(readset(q))
        line = dict(config=cfg, references=n, queries=nq, refdb_build_s=round(build_s, 3), **db.info())
        call = lambda: api.classify_search(db, dev, top_k=args.top_k, min_shared=args.min_shared)
        got = call()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter(); call(); ts.append(time.perf_counter() - t0)
        api.profile_enable(True); call(); prof, _ = api.profile_read(); api.profile_enable(False)
        line["classify_search_ms"] = round(float(np.median(ts)) * 1e3, 2)
        line["classify_search_runs_ms"] = [round(x * 1e3, 2) for x in ts]
        line["kernels_ms"] = {k_: round(v_[1], 3) for k_, v_ in prof.items() if k_.startswith(("k_classify", "k_hpc_minimizers", "hipcub_classify"))}
        line["kernel_launches"] = {k_: v_[0] for k_, v_ in prof.items() if k_.startswith("k_classify")}
        line["not_in_a_kernel_ms"] = round(line["classify_search_ms"] - sum(line["kernels_ms"].values()), 2)      # zeroing the count rows, copies, host work
        line["top1_is_the_member"] = round(float((got[0][:, 0] == member).mean()), 4); line["top1_strand_is_planted"] = round(float((got[2][:, 0] == rc).mean()), 4)
        if ref_rate is None:                                                          # the comparator, once
            rn, rq = min(args.ref_refs, n), min(args.ref_queries, nq)
            strs = lambda a: [r.tobytes().decode() for r in a]
            t0 = time.perf_counter(); want = ref.search(api, strs(rows[:rn]), strs(q[:rq]), 13, 20, args.top_k, args.min_shared); sec = time.perf_counter() - t0
            ref_rate = rn * rq / sec
            line["reference_measured"] = dict(references=rn, queries=rq, seconds=round(sec, 2))
            if rn == n:
                line["reference_equal_on_its_queries"] = bool(all(np.array_equal(a[:rq], b) for a, b in zip(got, want[:3])))
        line["reference_s"] = round(n * nq / ref_rate, 1)
        line["reference_note"] = "extrapolated from the measured run by references x queries, not run"
        line["reference_over_device_call"] = round(line["reference_s"] * 1e3 / line["classify_search_ms"], 1)
        emit(line)
        dev.release(); db.release()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
