"""ctypes view of the C-ABI declared in include/ngsid.h (structs + call wrappers).

`Api` binds one shared library.  The product binds libngsid_hip.so (prefix ``ngsid_``, ctx first);
the tests bind the CPU oracle with the same wrapper (prefix ``ongsid_``, no ctx) - the oracle is
never bound from inside this package.
"""
from __future__ import annotations
import os
import ctypes as C
from time import perf_counter as _perf
import numpy as np

MEM_HOST, MEM_DEVICE = 0, 1
ERRORS = {-1: "NGSID_ERR_NO_DEVICE", -2: "NGSID_ERR_ARG", -3: "NGSID_ERR_ALPHABET", -4: "NGSID_ERR_CAPACITY",
          -5: "NGSID_ERR_HIP", -6: "NGSID_ERR_TOO_LONG", -7: "NGSID_ERR_NO_PTABLE"}
ST_NEWREP, ST_MAPPED, ST_ALIGNED, ST_SHORT, ST_SEEDED = 0, 1, 2, 3, 4
POA_LOCAL, POA_GLOBAL, POA_SEMI = 0, 1, 2


class NgsidError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "NGSID_ERR"), code, text))
        self.code = code


class Reads(C.Structure):
    _fields_ = [("seq", C.c_void_p), ("qual", C.c_void_p), ("off", C.c_void_p), ("n", C.c_uint64), ("mem", C.c_uint32), ("_pad", C.c_uint32)]


class ClusterParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("w", C.c_int32), ("min_shared", C.c_int32), ("symmetric", C.c_int32),
                ("min_fraction", C.c_double), ("mapped_threshold", C.c_double), ("aligned_threshold", C.c_double),
                ("min_prob_no_hits", C.c_double), ("p_shared", C.c_double * 225)]


class PoaParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("match", C.c_int32), ("mismatch", C.c_int32), ("gap", C.c_int32),
                ("tile_depth", C.c_int32), ("band", C.c_int32), ("node_cap", C.c_int32), ("trim", C.c_int32), ("single_below", C.c_int32)]


class PolishParams(C.Structure):
    _fields_ = [("iters", C.c_int32), ("window", C.c_int32), ("quality_threshold", C.c_double), ("error_threshold", C.c_double),
                ("match", C.c_int32), ("mismatch", C.c_int32), ("gap", C.c_int32), ("k", C.c_int32), ("w", C.c_int32),
                ("tile_depth", C.c_int32), ("band", C.c_int32), ("node_cap", C.c_int32),
                ("aln_match", C.c_int32), ("aln_mismatch", C.c_int32), ("aln_open", C.c_int32), ("aln_ext", C.c_int32), ("trim", C.c_int32), ("aln_mode", C.c_int32), ("stop_when_stable", C.c_int32), ("single_below", C.c_int32)]


class SupportParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("w", C.c_int32), ("clip", C.c_int32)]          # include/ngsid_support.h ngsid_support_params_t


class DemuxParams(C.Structure):
    _fields_ = [("window", C.c_int32), ("max_ed", C.c_int32), ("iupac", C.c_int32)]  # include/ngsid_demux.h ngsid_demux_params_t


class DemuxScanParams(C.Structure):
    _fields_ = [("max_ed", C.c_int32), ("iupac", C.c_int32)]                         # include/ngsid_demux.h ngsid_demux_scan_params_t


class RefDbParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("w", C.c_int32)]                                  # include/ngsid_classify.h ngsid_refdb_params_t


class UmiParams(C.Structure):
    _fields_ = [("max_dist", C.c_int32), ("seed_len", C.c_int32)]                    # include/ngsid_umi.h ngsid_umi_params_t


class ClassifyParams(C.Structure):
    _fields_ = [("top_k", C.c_int32), ("min_shared", C.c_int32)]                     # include/ngsid_classify.h ngsid_classify_params_t


CLASSIFY_MAX_TOPK, CLASSIFY_MAX_K = 64, 21


CHIMERA_FIELDS = ("one_pair", "one_cost", "two_cost", "pair_a", "pair_b", "bp_lo", "bp_hi")   # the seven integers per query of Api.chimera_model (include/ngsid_chimera.h)
CHIMERA_NFIELD, CHIMERA_ROWS, CHIMERA_LDS_QUERY = 7, 12, 2048                      # NGSID_CHIMERA_NFIELD, _ROWS (R of k_chimera_profile), _LDS_QUERY
CHIMERA_STRIP = 64 * CHIMERA_ROWS                                                   # NGSID_CHIMERA_STRIP: parent rows per pass of a wave
MAX_CONSENSUS_LEN = 16384                                                           # include/ngsid.h NGSID_MAX_CONSENSUS_LEN
NEAR_MAX_DIST, NEAR_BOTH_STRANDS = 31, 1                                            # include/ngsid_near.h NGSID_NEAR_MAX_DIST, NGSID_NEAR_BOTH_STRANDS
NEAR_WIDE_MAX_DIST = 255                                                            # include/ngsid_near.h NGSID_NEAR_WIDE_MAX_DIST
UMI_MAX_LEN, UMI_MAX_DIST = 64, 8                                                   # include/ngsid_umi.h NGSID_UMI_MAX_LEN, NGSID_UMI_MAX_DIST
RECRUIT_MAX_LEN, RECRUIT_NFIELD, RECRUIT_BOTH_STRANDS = 2048, 6, 1                  # include/ngsid_recruit.h NGSID_RECRUIT_MAX_LEN, _NFIELD, _BOTH_STRANDS
RECRUIT_FIELDS = ("cons", "ed", "strand", "end", "cons2", "ed2")                    # the six integers per read of Api.recruit


def chimera_profile_offsets(query_lens, pair_off):
    """-> prof_off [n_pairs + 1] uint64: where the block of pair k (F_k[0 .. n] then B_k[0 .. n], n = its query's length) starts in the profiles of Api.chimera_model"""
    po = np.asarray(pair_off).astype(np.int64)
    cnt = np.maximum(np.diff(po), 0)
    off = np.zeros(int(cnt.sum()) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.repeat(2 * (np.asarray(query_lens).astype(np.int64) + 1), cnt))
    return off


DEMUX_FIELDS = ("tag", "ed", "start", "end", "ed2")                                # the five integers per (read, side) of Api.demux_locate
DEMUX_MAX_TAG_LEN, DEMUX_MAX_WINDOW = 64, 256
DEMUX_SCAN_FIELDS = ("pattern", "end", "ed")                                       # the three integers per hit of Api.demux_scan


SUPPORT_COLUMNS = ("depth", "agree", "A", "C", "G", "T", "del", "ins_after")       # the eight counters per base of Api.consensus_support


PHASE_MAX_SITES, PHASE_MAX_HAPS = 64, 16                                          # include/ngsid_phase.h
GENO_DEL, GENO_OTHER, GENO_NONE, HAP_ANY = 4, 5, 7, 255


def phase_offsets(grp_off, site_off):
    """-> (geno_off, tab_off) [n_groups + 1] uint64: where group g's [R_g, S_g] genotype block and its [S_g, S_g, 5, 5] pair tables start (include/ngsid_phase.h)"""
    r = np.diff(np.asarray(grp_off).astype(np.int64)); s = np.diff(np.asarray(site_off).astype(np.int64))
    geno_off = np.zeros(len(r) + 1, dtype=np.uint64); tab_off = np.zeros(len(r) + 1, dtype=np.uint64)
    geno_off[1:] = np.cumsum(r * s); tab_off[1:] = np.cumsum(25 * s * s)
    return geno_off, tab_off


HP_NBUCKET, HP_OTHER = 17, 16                                                      # include/ngsid_hp.h: buckets 0 - 14 exact run lengths, 15 = 15 or more, 16 = spanned, no length


CIGAR_NFIELD, CIGAR_MERGE_M = 5, 1                                                 # include/ngsid_cigar.h NGSID_CIGAR_NFIELD, NGSID_CIGAR_MERGE_M
CIGAR_FIELDS = ("t_begin", "t_end", "q_begin", "q_end", "nm")                      # the five integers per listed read of Api.read_cigars
CIGAR_OPS = "MIDNSHP=X"                                                            # BAM's op codes: an entry of ops is length << 4 | code


ERRPROF_NCOUNT, ERRPROF_NQ = 96, 94                                                # include/ngsid_errprof.h NGSID_ERRPROF_NCOUNT, _NQ
ERRPROF_PAIR, ERRPROF_INS_LETTER, ERRPROF_CEN_OTHER, ERRPROF_READS, ERRPROF_INS_LEN, ERRPROF_DEL_LEN, ERRPROF_HPCTX = 0, 24, 29, 30, 32, 48, 64      # where the tables of Api.error_profile start


def cluster_params(k=13, w=20, min_shared=5, min_fraction=0.8, mapped_threshold=0.7, aligned_threshold=0.4,
                   min_prob_no_hits=0.1, symmetric=False, p_shared=None):
    p = ClusterParams()
    p.k, p.w, p.min_shared, p.symmetric = int(k), int(w), int(min_shared), int(bool(symmetric))
    p.min_fraction, p.mapped_threshold, p.aligned_threshold, p.min_prob_no_hits = min_fraction, mapped_threshold, aligned_threshold, min_prob_no_hits
    t = np.full(225, np.nan) if p_shared is None else np.asarray(p_shared, dtype=np.float64)
    for i in range(225):
        p.p_shared[i] = t[i]
    return p


def poa_params(mode=POA_LOCAL, match=5, mismatch=-4, gap=-2, tile_depth=0, band=0, node_cap=0, trim=0, single_below=0):
    """Defaults = `spoa -l 0 -r 0 -g -2` (consensus.py:87; spoa 4.0.x m=5 n=-4, linear because g>=e)."""
    return PoaParams(int(mode), int(match), int(mismatch), int(gap), int(tile_depth), int(band), int(node_cap), int(trim), int(single_below))


ALN_SUBGRAPH = 16      # include/ngsid.h NGSID_ALN_SUBGRAPH: flag bit of aln_mode (racon's sub-graph alignment of the layers that do not span their window)


def polish_params(iters=2, window=500, quality_threshold=10.0, error_threshold=0.3, match=3, mismatch=-5, gap=-4,
                  k=13, w=20, tile_depth=0, band=0, node_cap=0, aln_match=2, aln_mismatch=-2, aln_open=3, aln_ext=1, trim=1, aln_mode=2, stop_when_stable=1, single_below=0,
                  subgraph_layers=False):
    """Defaults = racon 1.4.x (-w 500 -q 10 -e 0.3 -m 3 -x -5 -g -4), iters = --racon_iter (NGSpeciesID:212).
    subgraph_layers: ORs ALN_SUBGRAPH into aln_mode."""
    mode = int(aln_mode) | (ALN_SUBGRAPH if subgraph_layers else 0)
    return PolishParams(int(iters), int(window), float(quality_threshold), float(error_threshold), int(match), int(mismatch), int(gap),
                        int(k), int(w), int(tile_depth), int(band), int(node_cap), int(aln_match), int(aln_mismatch), int(aln_open), int(aln_ext), int(trim), mode, int(stop_when_stable), int(single_below))


class ReadSet:
    """CSR read set backed by numpy arrays (host) or by raw device pointers (torch tensors kept alive by the caller)."""

    def __init__(self, seq, qual, off, mem=MEM_HOST, keep=None):
        self.mem = mem
        self.keep = keep
        if mem == MEM_HOST:
            self.seq = np.ascontiguousarray(seq, dtype=np.uint8)
            self.qual = None if qual is None else np.ascontiguousarray(qual, dtype=np.uint8)
            self.off = np.ascontiguousarray(off, dtype=np.uint64)
            self.n = len(self.off) - 1
            self.c = Reads(self.seq.ctypes.data, None if self.qual is None else self.qual.ctypes.data, self.off.ctypes.data, self.n, MEM_HOST, 0)
        else:
            self.seq, self.qual, self.off = seq, qual, off            # integers (device addresses)
            self.n = int(keep["n"])
            self.c = Reads(int(seq), None if qual is None else int(qual), int(off), self.n, MEM_DEVICE, 0)

    @staticmethod
    def from_strings(seqs, quals=None):
        off = np.zeros(len(seqs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        seq = np.frombuffer("".join(seqs).encode(), dtype=np.uint8).copy() if len(seqs) else np.zeros(0, np.uint8)
        qual = None
        if quals is not None:
            qual = np.frombuffer("".join(quals).encode(), dtype=np.uint8).copy() if len(quals) else np.zeros(0, np.uint8)
        return ReadSet(seq, qual, off)

    @staticmethod
    def from_torch(seq_t, qual_t, off_t):
        """torch tensors on a cuda/hip device: uint8, uint8, int64 (n+1).  The library works on its own HIP stream, so torch's stream
        is drained first: whatever produced the tensors must have finished writing them before the hand-over."""
        import torch
        torch.cuda.current_stream(seq_t.device).synchronize()
        keep = dict(seq=seq_t, qual=qual_t, off=off_t, n=off_t.numel() - 1)
        return ReadSet(seq_t.data_ptr(), None if qual_t is None else qual_t.data_ptr(), off_t.data_ptr(), MEM_DEVICE, keep)

    def release(self):
        """device read set made by Api.upload_reads: give the buffers back (idempotent)"""
        k = self.keep if isinstance(self.keep, dict) else None
        if self.mem == MEM_DEVICE and k and k.get("api") is not None:
            api, k["api"] = k["api"], None
            api._call("reads_release", C.byref(self.c))

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def get(self, i):
        a, b = int(self.off[i]), int(self.off[i + 1])
        return self.seq[a:b].tobytes().decode(), (None if self.qual is None else self.qual[a:b].tobytes().decode())


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _p0(a):
    """_p of a list the C-ABI takes no null for: an empty array is passed as one zero element of its dtype"""
    return None if a is None else _p(a if len(a) else np.zeros(1, a.dtype))


def _groups(grp_off, read_order):
    """-> (grp_off uint64, read_order uint32 or None, n_groups) as the C-ABI takes them"""
    grp_off = np.ascontiguousarray(grp_off, dtype=np.uint64)
    return grp_off, None if read_order is None else np.ascontiguousarray(read_order, dtype=np.uint32), len(grp_off) - 1


def _strings(buf, off, n):
    """the n strings of a CSR result (bytes buf, offsets off)"""
    return [buf[int(off[i]):int(off[i + 1])].tobytes().decode() for i in range(n)]


def _as_reads(x):
    return x if isinstance(x, ReadSet) else ReadSet.from_strings(list(x))


def _consensus_cap(rs, ng):
    """bytes for the consensuses of ng groups: four times the longest read each (a host set tells its lengths)"""
    lens = np.diff(rs.off.astype(np.int64)) if rs.mem == MEM_HOST else None
    return int(4 * (lens.max() if lens is not None and len(lens) else 16384) * max(ng, 1) + 1024)


def _polish_cap(backbones):
    return int(4 * len(backbones.seq) + 4096) if backbones.mem == MEM_HOST else 1 << 24


LANES = int(os.environ.get("NGSID_LANES", "2"))           # contexts a consensus / polishing call is dealt to (Api.lanes); 1 = off
LANE_MIN_READS = 100_000                                   # below: one context (measured on the bench workload: 100 k reads 109.5 ms either way, 300 k reads 248 -> 242 ms, 1 M 719 -> 708 ms)
LANE_MAX_READS = 4_000_000                                 # above: one context (a second one doubles the grow-only scratch: 130 - 140 GB at 10 M reads)


def lane_deal(sizes, lanes):
    """groups -> lanes: largest first to the lightest lane; per lane the group numbers ascending"""
    load = [0] * lanes; deal = [[] for _ in range(lanes)]
    for g in sorted(range(len(sizes)), key=lambda g: (-int(sizes[g]), g)):
        x = int(np.argmin(load))
        deal[x].append(g); load[x] += int(sizes[g])
    return [sorted(d) for d in deal if d]


def _lane_lists(grp_off, read_order, gs):
    """(grp_off, read_order) of the groups gs of a call"""
    go = np.asarray(grp_off, dtype=np.int64)
    off = np.zeros(len(gs) + 1, dtype=np.uint64); off[1:] = np.cumsum([int(go[g + 1] - go[g]) for g in gs])
    if read_order is None:
        ro = np.concatenate([np.arange(go[g], go[g + 1], dtype=np.uint32) for g in gs])
    else:
        r = np.asarray(read_order); ro = np.concatenate([r[int(go[g]):int(go[g + 1])] for g in gs]).astype(np.uint32)
    return off, ro


def _lane_backbones(bb: "ReadSet", gs):
    o = bb.off.astype(np.int64)
    off = np.zeros(len(gs) + 1, dtype=np.uint64); off[1:] = np.cumsum([int(o[g + 1] - o[g]) for g in gs])
    seq = np.concatenate([bb.seq[int(o[g]):int(o[g + 1])] for g in gs]) if len(gs) else np.zeros(0, np.uint8)
    qual = None if bb.qual is None else np.concatenate([bb.qual[int(o[g]):int(o[g + 1])] for g in gs])
    return ReadSet(seq, qual, off)


class LaneRecords:
    """alignment records [it][x][6] of a polish_trace(aln=True) call that ran in lanes: rec[it][a:b] of ONE group's range (what the PAF writers take) is a view into that lane's
    array; anything else goes through the merged array, built on first use (72 MB per million reads and three iterations: not copied unless somebody asks)"""
    def __init__(self, go, iters, where):
        self.go, self.iters, self.where, self._all = go, iters, where, None
        self.shape = (iters, int(go[-1]), 6); self._start = {int(go[g]): g for g in range(len(go) - 1)}

    def __array__(self, dtype=None, copy=None):
        if self._all is None:
            self._all = np.empty(self.shape, dtype=np.int32)
            for g, (arr, pos, n) in enumerate(self.where): self._all[:, int(self.go[g]):int(self.go[g + 1])] = arr[:, pos:pos + n]
        return self._all if dtype is None else self._all.astype(dtype)

    def __len__(self):
        return self.iters

    def __getitem__(self, i):
        if isinstance(i, (int, np.integer)): return _LaneRecordsOfIteration(self, int(i))
        return np.asarray(self)[i]


class _LaneRecordsOfIteration:
    def __init__(self, parent, it): self.p, self.it = parent, it

    def __array__(self, dtype=None, copy=None):
        a = np.asarray(self.p)[self.it]; return a if dtype is None else a.astype(dtype)

    def __getitem__(self, sl):
        p = self.p
        if isinstance(sl, slice) and sl.step in (None, 1) and sl.start is not None and sl.stop is not None:
            g = p._start.get(int(sl.start))
            if g is not None and int(p.go[g + 1]) == int(sl.stop):
                arr, pos, n = p.where[g]; return arr[self.it, pos:pos + n]
        return np.asarray(p)[self.it][sl]


class Api:
    def __init__(self, lib: C.CDLL, prefix: str, ctx=None):
        self.lib, self.prefix, self.ctx = lib, prefix, ctx
        self.has_ctx = ctx is not None

    def close(self):
        """ngsid_destroy: releases the context's stream, side streams, pinned staging and scratch buffers (and, with the last context of the
        process, the device-memory cache and the read sets uploaded through it).  Contexts from runtime.get_api() are shared and stay open;
        the ones from runtime.new_api() belong to their caller: close them (or use `with runtime.new_api() as api:`)."""
        for t, ex in self.__dict__.pop("_twin_list", []):
            ex.shutdown(wait=True); t.close()
        if self.has_ctx and self.ctx is not None:
            f = getattr(self.lib, self.prefix + "destroy"); f.restype = None
            f(self.ctx)
            self.ctx = None; self.has_ctx = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _fn(self, name):
        f = getattr(self.lib, self.prefix + name)
        f.restype = C.c_int32
        return f

    def _call(self, name, *args):
        f = self._fn(name)
        t0 = _perf()
        rc = f(self.ctx, *args) if self.has_ctx else f(*args)
        cs = self.__dict__.setdefault("call_s", {})        # wall time per entry point as THIS side sees it (ctypes call + the wait for the interpreter lock on return); the library's
        cs[name] = cs.get(name, 0.0) + _perf() - t0        # own clock for the same calls: "host_<name>" lines of ngsid_profile_read (bench.py config.cli.binding_overhead_s)
        return rc

    # ---- lanes (round 6): the groups of ONE consensus / polishing call are independent, so they are dealt to `lanes` contexts of the same device, each driven by its own long-lived
    # host thread on its own HIP stream.  One lane's kernels then run in the other's host gaps (the unit and tile lists between the aligner and the POA levels of every polishing
    # iteration: ~3 ms each, GPU idle) and under the latency-bound top levels of its hierarchy.  Same results group by group (tests run both ways).  lanes = 1: off.
    lanes = LANES

    def _lane_deal(self, rs, grp_off, backbones=None):
        """-> per lane the (ascending) group numbers, or None when the call runs in this context alone"""
        ng = len(grp_off) - 1
        if self.lanes < 2 or ng < 2 or not self.has_ctx or self.prefix != "ngsid_" or "device" not in self.__dict__ or rs.mem != MEM_DEVICE or (backbones is not None and backbones.mem != MEM_HOST):
            return None
        sizes = np.diff(np.asarray(grp_off, dtype=np.int64))
        if not (LANE_MIN_READS <= int(sizes.sum()) <= LANE_MAX_READS):
            return None
        deal = lane_deal(sizes, min(self.lanes, ng))
        try:
            self._twins(len(deal) - 1)
        except NgsidError:                # no second context to be had (memory): this one does the work, from now on
            self.lanes = 1
            return None
        return deal

    def set_option(self, name, value):
        """ngsid_ctx_option on this context and on its lane contexts (present and future)"""
        self.__dict__.setdefault("_options", {})[name] = int(value)
        for a in self.contexts():
            if a.lib.ngsid_ctx_option(a.ctx, name.encode(), C.c_int64(int(value))) != 0: a._err(-2)

    def _twins(self, n):
        tw = self.__dict__.setdefault("_twin_list", [])
        while len(tw) < n:
            from . import runtime
            from concurrent.futures import ThreadPoolExecutor
            # ONE long-lived thread per twin: the library keeps its pinned staging vectors per host thread; a fresh thread per call would allocate them again every time, and
            # releasing pinned memory waits for the whole device - i.e. for the other lane
            opts = dict(self.__dict__.get("_options", {}))
            opts.setdefault("scratch_budget_mb", 16384)          # half the default aligner-traceback budget (measured: same speed - the lanes share the device anyway -, C5 at 2 M reads 204 -> 177 GB with both contexts at 16 GB)
            tw.append((runtime.new_api(self.__dict__.get("device"), options=opts), ThreadPoolExecutor(max_workers=1, thread_name_prefix="ngsid-lane")))
            tw[-1][0].lanes = 1
        return tw[:n]

    def _lane_run(self, deal, fn):
        tw = self._twins(len(deal) - 1)
        futs = [tw[x - 1][1].submit(fn, tw[x - 1][0], deal[x]) for x in range(1, len(deal))]
        try:
            res = [fn(self, deal[0])]
        finally:
            excs = [f.exception() for f in futs]          # (waits for every lane, whatever happened here)
        for e in excs:
            if e is not None: raise e
        return res + [f.result() for f in futs]

    def _lanes_or_none(self, deal, fn):
        """the lanes' results, or None when a lane ran out of device memory (a second context's working set did not fit beside the first): the lane contexts give their
        memory back, this context does the call alone - now (the caller repeats it) and from now on"""
        try:
            return self._lane_run(deal, fn)
        except NgsidError as e:
            if "out of memory" not in str(e).lower(): raise
            self.lanes = 1
            for t, _ in self.__dict__.get("_twin_list", []):
                try: t.lib.ngsid_ctx_option(t.ctx, b"release_scratch", C.c_int64(1))
                except Exception: pass
            return None

    def contexts(self):
        """this context and the lane contexts it has made (profiling and statistics are per context)"""
        return [self] + [t[0] for t in self.__dict__.get("_twin_list", [])]

    def profile_enable(self, on: bool):
        """ngsid_profile_enable on this context and its lane contexts"""
        for a in self.contexts(): a.lib.ngsid_profile_enable(a.ctx, C.c_int32(1 if on else 0))

    def profile_read(self):
        """ngsid_profile_read of this context and its lane contexts -> ({name: (count, ms)} summed, [the same per context]).  Kernel lines are HIP-event brackets of every launch
        on its own stream: launches of two lanes that overlap on the device are both counted in full."""
        per = []
        for a in self.contexts():
            buf = C.create_string_buffer(1 << 16); a.lib.ngsid_profile_read(a.ctx, buf, C.c_uint64(len(buf)))
            d = {}
            for line in buf.value.decode().splitlines():
                nm, cnt, ms = line.split(); d[nm] = (int(cnt), float(ms))
            per.append(d)
        tot = {}
        for d in per:
            for nm, (c_, m_) in d.items():
                c0, m0 = tot.get(nm, (0, 0.0)); tot[nm] = (c0 + c_, m0 + m_)
        return tot, per

    def upload_reads(self, rs: "ReadSet") -> "ReadSet":
        """host read set -> device-resident read set (one PCIe copy for all the calls that follow); backends without the entry point
        (the test oracle) and read sets that are on the device already are returned as they are"""
        if rs.mem != MEM_HOST or not hasattr(self.lib, self.prefix + "reads_upload"):
            return rs
        out = Reads()
        rc = self._call("reads_upload", C.byref(rs.c), C.byref(out))
        if rc: self._err(rc)
        return ReadSet(out.seq, out.qual, out.off, MEM_DEVICE, dict(n=rs.n, api=self, host=rs))

    def reads_subset(self, dev: "ReadSet", idx):
        """reads idx (in that order) of a device-resident read set -> (new device-resident read set, number of bases outside ACGTN in it); None when the backend
        has no such entry point (the test oracle) or the set is on the host"""
        if dev.mem != MEM_DEVICE or not hasattr(self.lib, self.prefix + "reads_subset"):
            return None
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        out = Reads(); foreign = C.c_uint64(0)
        rc = self._call("reads_subset", C.byref(dev.c), _p(idx), C.c_uint64(len(idx)), C.byref(out), C.byref(foreign))
        if rc: self._err(rc)
        return ReadSet(out.seq, out.qual, out.off, MEM_DEVICE, dict(n=len(idx), api=self)), int(foreign.value)

    def _err(self, rc):
        g = getattr(self.lib, self.prefix + "last_error"); g.restype = C.c_char_p
        txt = g(self.ctx) if self.has_ctx else g()
        raise NgsidError(rc, (txt or b"").decode(errors="replace"))

    def _need(self, header, *names):
        if not all(hasattr(self.lib, self.prefix + n) for n in names):
            raise NgsidError(-2, "the bound library does not export %s (include/%s): rebuild it from this tree" % (" / ".join(self.prefix + n for n in names), header))

    def _found_list(self, entry, head, n_out, alloc, cap, tail=()):
        """the count-then-fill protocol of a call that returns a list of unknown length: entry(*head, *outputs, cap, *tail, &needed).  cap None: the count call (no
        outputs, cap 0; NGSID_ERR_CAPACITY is its answer whenever something was found), then the fill call with room for what it counted; a cap: that fill call alone.
        alloc(cap) -> the n_out output arrays.  -> (outputs, needed); a capacity error of the fill call carries .needed"""
        needed = C.c_uint64(0)
        if cap is None:
            rc = self._call(entry, *head, *[None] * n_out, C.c_uint64(0), *tail, C.byref(needed))
            if rc and rc != -4: self._err(rc)
            cap = needed.value
        outs = alloc(int(cap))
        rc = self._call(entry, *head, *[_p(a) for a in outs], C.c_uint64(int(cap)), *tail, C.byref(needed))
        if rc:
            try: self._err(rc)
            except NgsidError as e:
                e.needed = int(needed.value); raise
        return outs, int(needed.value)

    def _support_head(self, what, header, names, centres, grp_off, read_order, k, w, clip):
        """what consensus_support, hp_runs and phase_genotypes begin with: the centres are a host set, the entry points exist -> (grp_off, read_order, n_groups as the
        C-ABI takes them, strand [n_listed] int8 filled with -1, SupportParams)"""
        if centres.mem != MEM_HOST: raise ValueError("%s takes the centres as a host read set" % what)
        self._need(header, *names)
        grp_off, ro, ng = _groups(grp_off, read_order)
        return grp_off, ro, ng, np.full(max(int(grp_off[-1]), 1), -1, dtype=np.int8), SupportParams(int(k), int(w), 1 if clip else 0)

    # ---- (f1)
    def score_reads(self, rs: ReadSet, k, q_threshold=7.0):
        n = rs.n
        score = np.zeros(n); err = np.zeros(n); keep = np.zeros(n, dtype=np.uint8)
        rc = self._call("score_reads", C.byref(rs.c), C.c_int32(k), C.c_double(q_threshold), _p(score), _p(err), _p(keep))
        if rc: self._err(rc)
        return score, err, keep

    # ---- (a1-a3)
    def hpc_minimizers(self, rs: ReadSet, k, w, cap=None):
        assert rs.mem == MEM_HOST, "host wrapper; device callers use the raw C-ABI"
        n = rs.n
        if cap is None:
            cap = max(16, int(len(rs.seq)))
        moff = np.zeros(n + 1, dtype=np.uint64); codes = np.zeros(cap, dtype=np.uint64); pos = np.zeros(cap, dtype=np.uint32)
        hl = np.zeros(n, dtype=np.uint32); he = np.zeros(n); needed = C.c_uint64(0)
        rc = self._call("hpc_minimizers", C.byref(rs.c), C.c_int32(k), C.c_int32(w), _p(moff), _p(codes), _p(pos), C.c_uint64(cap), C.byref(needed), _p(hl), _p(he))
        if rc: self._err(rc)
        t = int(moff[-1])
        return moff, codes[:t], pos[:t], hl, he

    # ---- (a4-a11)
    def cluster_greedy(self, rs: ReadSet, prm: ClusterParams, acc_rank=None, prev_batch=None, known_err=None):
        n = rs.n
        rep = np.zeros(n, dtype=np.int32); herr = np.zeros(n); st = np.zeros(n, dtype=np.uint8); cnt = np.zeros(4, dtype=np.uint64)
        ar = None if acc_rank is None else np.ascontiguousarray(acc_rank, dtype=np.uint32)
        pb = None if prev_batch is None else np.ascontiguousarray(prev_batch, dtype=np.int32)
        ke = None if known_err is None else np.ascontiguousarray(known_err, dtype=np.float64)
        rc = self._call("cluster_greedy", C.byref(rs.c), C.byref(prm), _p(ar), _p(pb), _p(ke), _p(rep), _p(herr), _p(st), _p(cnt))
        if rc: self._err(rc)
        return rep, herr, st, cnt

    def cluster_greedy_segmented(self, rs: ReadSet, prm: ClusterParams, seg_off, acc_rank=None):
        """include/ngsid_batch.h: reads [seg_off[s], seg_off[s+1]) are sample s, clustered as if alone -> (rep_of, herr, status, counters[n_segments, 4]), rep_of
        indexing the whole set.  A library without the entry point (the test oracle) runs cluster_greedy once per segment: that loop is the definition of the call."""
        n = rs.n
        so = np.ascontiguousarray(seg_off, dtype=np.uint64); ns = len(so) - 1
        ar = None if acc_rank is None else np.ascontiguousarray(acc_rank, dtype=np.uint32)
        rep = np.zeros(n, dtype=np.int32); herr = np.zeros(n); st = np.zeros(n, dtype=np.uint8); cnt = np.zeros((max(ns, 0), 4), dtype=np.uint64)
        if hasattr(self.lib, self.prefix + "cluster_greedy_segmented"):
            if ns < 0: self._seg_err("seg_off is empty")
            rc = self._call("cluster_greedy_segmented", C.byref(rs.c), C.byref(prm), _p(ar), _p(so), C.c_uint64(ns), _p(rep), _p(herr), _p(st), _p(cnt))
            if rc: self._err(rc)
            return rep, herr, st, cnt
        if ns < 0 or int(so[0]) != 0 or int(so[-1]) != n or (np.diff(so.astype(np.int64)) < 0).any():
            self._seg_err("seg_off must start at 0, end at the number of reads and not decrease")
        if rs.mem != MEM_HOST: raise ValueError("the per-segment fallback takes a host read set")
        from .hostutil import subset_reads
        for s in range(ns):
            a, b = int(so[s]), int(so[s + 1])
            if a == b: continue
            r, h, t, c = self.cluster_greedy(subset_reads(rs, np.arange(a, b)), prm, acc_rank=None if ar is None else ar[a:b])
            rep[a:b] = r + a; herr[a:b] = h; st[a:b] = t; cnt[s] = c
        return rep, herr, st, cnt

    @staticmethod
    def _seg_err(text):
        raise NgsidError(-2, text)

    def merge_representatives(self, reps: ReadSet, prm: ClusterParams, score, hpc_err, batch, n_batches, acc_rank=None):
        """merge rounds of parallel_clustering on gathered representatives -> rep_of [R] (index of the final representative)"""
        R = reps.n
        rep = np.zeros(R, dtype=np.int32)
        sc = np.ascontiguousarray(score, dtype=np.float64); he = np.ascontiguousarray(hpc_err, dtype=np.float64); bt = np.ascontiguousarray(batch, dtype=np.int32)
        ar = None if acc_rank is None else np.ascontiguousarray(acc_rank, dtype=np.uint32)
        rc = self._call("merge_representatives", C.byref(reps.c), C.byref(prm), _p(ar), _p(sc), _p(he), _p(bt), C.c_int32(int(n_batches)), _p(rep))
        if rc: self._err(rc)
        return rep

    # ---- (a10,a15)
    def sg_align_batch(self, q: ReadSet, t: ReadSet, q_idx, t_idx, open_, ext=1, match=2, mismatch=-2, k=13, match_id=None):
        q_idx = np.ascontiguousarray(q_idx, dtype=np.uint32); t_idx = np.ascontiguousarray(t_idx, dtype=np.uint32)
        n = len(q_idx)
        open_ = np.ascontiguousarray(np.broadcast_to(np.asarray(open_, dtype=np.int32), (n,)))
        mid = np.ascontiguousarray(np.broadcast_to(np.asarray(k if match_id is None else match_id, dtype=np.int32), (n,)))
        score = np.zeros(n, dtype=np.int32); ncols = np.zeros(n, dtype=np.int32); nmatch = np.zeros(n, dtype=np.int32); region = np.zeros(n, dtype=np.int32)
        rc = self._call("sg_align_batch", C.byref(q.c), C.byref(t.c), _p(q_idx), _p(t_idx), C.c_uint64(n), C.c_int32(match), C.c_int32(mismatch),
                        _p(open_), C.c_int32(ext), C.c_int32(k), _p(mid), _p(score), _p(ncols), _p(nmatch), _p(region))
        if rc: self._err(rc)
        return score, ncols, nmatch, region

    def sg_align_cigar_batch(self, q: ReadSet, t: ReadSet, q_idx, t_idx, open_, ext=1, match=2, mismatch=-2):
        """-> (score [n], list of column strings over '=XID' in alignment order, one per pair): the alignment parasail returns as a CIGAR"""
        q_idx = np.ascontiguousarray(q_idx, dtype=np.uint32); t_idx = np.ascontiguousarray(t_idx, dtype=np.uint32)
        n = len(q_idx)
        open_ = np.ascontiguousarray(np.broadcast_to(np.asarray(open_, dtype=np.int32), (n,)))
        ql = np.diff(q.off.astype(np.int64)); tl = np.diff(t.off.astype(np.int64))
        cap = int((ql[q_idx] + tl[t_idx]).sum()) + 1 if n else 1
        score = np.zeros(n, dtype=np.int32); off = np.zeros(n + 1, dtype=np.uint64); ops = np.zeros(cap, dtype=np.uint8); needed = C.c_uint64(0)
        rc = self._call("sg_align_cigar_batch", C.byref(q.c), C.byref(t.c), _p(q_idx), _p(t_idx), C.c_uint64(n), C.c_int32(match), C.c_int32(mismatch),
                        _p(open_), C.c_int32(ext), _p(score), _p(off), _p(ops), C.c_uint64(cap), C.byref(needed))
        if rc: self._err(rc)
        return score, _strings(ops, off, n)

    def ed_align_batch(self, q: ReadSet, t: ReadSet, q_idx, t_idx, window=500, bp_windows=0):
        """edit-distance (read inside backbone) alignment of the polisher: distance, span[n,4], bp[n,bp_windows,4]"""
        q_idx = np.ascontiguousarray(q_idx, dtype=np.uint32); t_idx = np.ascontiguousarray(t_idx, dtype=np.uint32)
        n = len(q_idx)
        dist = np.zeros(n, dtype=np.int32); span = np.zeros((n, 4), dtype=np.int32); bp = np.zeros((n, max(bp_windows, 1), 4), dtype=np.int32)
        rc = self._call("ed_align_batch", C.byref(q.c), C.byref(t.c), _p(q_idx), _p(t_idx), C.c_uint64(n), C.c_int32(window), C.c_int32(bp_windows),
                        _p(dist), _p(span), _p(bp) if bp_windows else None)
        if rc: self._err(rc)
        return dist, span, bp[:, :bp_windows]

    # ---- (a13,a14)
    def poa_consensus(self, rs: ReadSet, grp_off, prm: PoaParams, cap=None, read_order=None):
        deal = self._lane_deal(rs, grp_off) if cap is None else None
        if deal is None:
            return self._poa_consensus1(rs, grp_off, prm, cap, read_order)
        def one(a, gs):
            off, ro = _lane_lists(grp_off, read_order, gs)
            return a._poa_consensus1(rs, off, prm, None, ro)
        parts = self._lanes_or_none(deal, one)
        if parts is None: return self._poa_consensus1(rs, grp_off, prm, cap, read_order)
        out = [None] * (len(grp_off) - 1)
        for gs, r in zip(deal, parts):
            for x, g in enumerate(gs): out[g] = r[x]
        return out

    def _poa_call(self, name, rs, grp_off, prm, cap, read_order, *extra, cov=False):
        """one of the three ngsid_poa_consensus* calls (extra: the arguments between prm and the outputs) -> (consensus strings, coverage array or None, offsets)"""
        grp_off, ro, ng = _groups(grp_off, read_order)
        if cap is None: cap = _consensus_cap(rs, ng)
        coff = np.zeros(ng + 1, dtype=np.uint64); cons = np.zeros(cap, dtype=np.uint8); needed = C.c_uint64(0)
        cv = np.zeros(cap, dtype=np.uint32) if cov else None
        rc = self._call(name, C.byref(rs.c), _p(ro), _p(grp_off), C.c_uint64(ng), C.byref(prm), *extra, _p(coff), _p(cons), *([_p(cv)] if cov else []), C.c_uint64(cap), C.byref(needed))
        if rc: self._err(rc)
        return _strings(cons, coff, ng), cv, coff

    def _poa_consensus1(self, rs: ReadSet, grp_off, prm: PoaParams, cap=None, read_order=None):
        return self._poa_call("poa_consensus", rs, grp_off, prm, cap, read_order)[0]

    def poa_consensus_weighted(self, rs: ReadSet, grp_off, prm: PoaParams, weight, cap=None, read_order=None):
        """ngsid_poa_consensus_weighted: sequence i stands for weight[i] reads (the merge of per-shard partial consensuses)"""
        wv = np.ascontiguousarray(weight, dtype=np.uint32); assert len(wv) == rs.n
        return self._poa_call("poa_consensus_weighted", rs, grp_off, prm, cap, read_order, _p(wv))[0]

    def poa_consensus_cov(self, rs: ReadSet, grp_off, prm: PoaParams, cap=None, read_order=None):
        """-> [(consensus string, uint32 coverage array)] per group"""
        seqs, cov, coff = self._poa_call("poa_consensus_cov", rs, grp_off, prm, cap, read_order, cov=True)
        return [(s, cov[int(coff[g]):int(coff[g + 1])].copy()) for g, s in enumerate(seqs)]

    # ---- (a16,a17)
    def polish(self, backbones: ReadSet, rs: ReadSet, grp_off, prm: PolishParams, cap=None, read_order=None):
        deal = self._lane_deal(rs, grp_off, backbones) if cap is None else None
        if deal is None:
            return self._polish1(backbones, rs, grp_off, prm, cap, read_order)
        def one(a, gs):
            off, ro = _lane_lists(grp_off, read_order, gs)
            return a._polish1(_lane_backbones(backbones, gs), rs, off, prm, None, ro)
        parts = self._lanes_or_none(deal, one)
        if parts is None: return self._polish1(backbones, rs, grp_off, prm, cap, read_order)
        ng = len(grp_off) - 1; seqs = [None] * ng; used = np.zeros(ng, dtype=np.uint64)
        for gs, (sq, us) in zip(deal, parts):
            for x, g in enumerate(gs): seqs[g] = sq[x]; used[g] = us[x]
        return seqs, used

    def _polish1(self, backbones: ReadSet, rs: ReadSet, grp_off, prm: PolishParams, cap=None, read_order=None):
        grp_off, ro, ng = _groups(grp_off, read_order)
        if cap is None: cap = _polish_cap(backbones)
        ooff = np.zeros(ng + 1, dtype=np.uint64); out = np.zeros(cap, dtype=np.uint8); needed = C.c_uint64(0); used = np.zeros(max(ng, 1), dtype=np.uint64)
        rc = self._call("polish", C.byref(backbones.c), C.byref(rs.c), _p(ro), _p(grp_off), C.c_uint64(ng), C.byref(prm), _p(ooff), _p(out), C.c_uint64(cap), C.byref(needed), _p(used))
        if rc: self._err(rc)
        return _strings(out, ooff, ng), used[:ng]

    def polish_trace(self, backbones: ReadSet, rs: ReadSet, grp_off, prm: PolishParams, cap=None, read_order=None, aln=False):
        """ngsid_polish_trace: -> (seqs[it][g], used[it][g]): every group's sequence after every iteration (the last one is what polish() returns).
        aln=True (ngsid_polish_trace_aln): -> (seqs, used, aln[it][x] = (strand, q_begin, q_end, t_begin, t_end, distance) of listed read x) - the PAF records of every iteration."""
        deal = self._lane_deal(rs, grp_off, backbones) if cap is None else None
        if deal is None:
            return self._polish_trace1(backbones, rs, grp_off, prm, cap, read_order, aln)
        def one(a, gs):
            off, ro = _lane_lists(grp_off, read_order, gs)
            return a._polish_trace1(_lane_backbones(backbones, gs), rs, off, prm, None, ro, aln)
        go = np.asarray(grp_off, dtype=np.int64); ng = len(go) - 1; iters = int(prm.iters)
        parts = self._lanes_or_none(deal, one)
        if parts is None: return self._polish_trace1(backbones, rs, grp_off, prm, cap, read_order, aln)
        seqs = [[None] * ng for _ in range(iters)]; used = np.zeros((iters, ng), dtype=np.uint64); where = [None] * ng
        for gs, r in zip(deal, parts):
            pos = 0
            for x, g in enumerate(gs):
                n = int(go[g + 1] - go[g])
                for it in range(iters): seqs[it][g] = r[0][it][x]
                used[:, g] = r[1][:, x]
                if aln: where[g] = (r[2], pos, n)
                pos += n
        return (seqs, used, LaneRecords(go, iters, where)) if aln else (seqs, used)

    def _polish_trace1(self, backbones: ReadSet, rs: ReadSet, grp_off, prm: PolishParams, cap=None, read_order=None, aln=False):
        grp_off, ro, ng = _groups(grp_off, read_order); iters = int(prm.iters); n = iters * ng
        if cap is None: cap = _polish_cap(backbones) * max(iters, 1)
        ooff = np.zeros(n + 1, dtype=np.uint64); out = np.zeros(cap, dtype=np.uint8); needed = C.c_uint64(0); used = np.zeros(max(n, 1), dtype=np.uint64)
        if aln:
            nl = int(grp_off[-1]); rec = np.empty((iters, nl, 6), dtype=np.int32)
            rc = self._call("polish_trace_aln", C.byref(backbones.c), C.byref(rs.c), _p(ro), _p(grp_off), C.c_uint64(ng), C.byref(prm), _p(ooff), _p(out), C.c_uint64(cap), C.byref(needed), _p(used), _p(rec))
        else:
            rc = self._call("polish_trace", C.byref(backbones.c), C.byref(rs.c), _p(ro), _p(grp_off), C.c_uint64(ng), C.byref(prm), _p(ooff), _p(out), C.c_uint64(cap), C.byref(needed), _p(used))
        if rc: self._err(rc)
        flat = _strings(out, ooff, n); seqs = [flat[it * ng:(it + 1) * ng] for it in range(iters)]
        u = used[:n].reshape(iters, ng) if n else used[:0].reshape(0, ng)
        return (seqs, u, rec) if aln else (seqs, u)

    # ---- include/ngsid_support.h
    def consensus_support(self, centres: ReadSet, rs: ReadSet, grp_off, read_order=None, k=13, w=20, clip=False):
        """ngsid_consensus_support: per base of every centre how many of its group's reads agree, disagree (and with what), delete or insert ->
        (counts [total, 8] uint32 in SUPPORT_COLUMNS order, cen_off [n_groups + 1], n_used [n_groups], strand [n_listed] int8: 0, 1, -1 = no shared minimizer).
        Rows cen_off[g] .. cen_off[g + 1] of counts are centre g.  Grouping as in polish(); clip=True counts a read between its first and last run of 15 equal
        columns only (the polisher's aln_mode 3).  There is no CPU implementation: a library without the entry point is an error."""
        grp_off, ro, ng, strand, prm = self._support_head("consensus_support", "ngsid_support.h", ("consensus_support",), centres, grp_off, read_order, k, w, clip)
        cen_off = centres.off.copy(); total = int(cen_off[-1]) if len(cen_off) else 0
        counts = np.zeros((total, 8), dtype=np.uint32); used = np.zeros(max(ng, 1), dtype=np.uint64)
        rc = self._call("consensus_support", C.byref(centres.c), C.byref(rs.c), _p(ro), _p(grp_off), C.c_uint64(ng), C.byref(prm), _p(counts), _p(used), _p(strand))
        if rc: self._err(rc)
        return counts, cen_off, used[:ng], strand[:int(grp_off[-1])]

    # ---- include/ngsid_hp.h
    def hp_runs(self, centres: ReadSet, rs: ReadSet, grp_off, run_off, run_start, read_order=None, k=13, w=20, clip=False):
        """ngsid_hp_runs: how long the runs run_start[run_off[g]:run_off[g + 1]] (ascending first positions of maximal runs of equal bytes of centre g) are in the reads
        of the group -> (hist [n_runs, 2, HP_NBUCKET] uint32, strand [n_listed] int8).  hist[run_off[g] + r, s, l]: reads of strand s whose run, between two '=' flanks, has
        l bases of the run's letter and nothing else (l = 15: 15 or more); bucket HP_OTHER: reads that span the run without giving a length.  Grouping, strands and counted
        columns as in consensus_support().  There is no CPU implementation: a library without the entry point is an error."""
        grp_off, ro, ng, strand, prm = self._support_head("hp_runs", "ngsid_hp.h", ("hp_runs",), centres, grp_off, read_order, k, w, clip)
        run_off = np.ascontiguousarray(run_off, dtype=np.uint64); run_start = np.ascontiguousarray(run_start, dtype=np.uint32)
        if len(run_off) != ng + 1 or len(run_start) != int(run_off[-1]): raise ValueError("hp_runs: run_off has one entry per group + 1 and run_start run_off[-1] entries")
        nr = int(run_off[-1])
        hist = np.zeros((max(nr, 1), 2, HP_NBUCKET), dtype=np.uint32)
        rc = self._call("hp_runs", C.byref(centres.c), C.byref(rs.c), _p(ro), _p(grp_off), C.c_uint64(ng), C.byref(prm), _p(run_off), _p0(run_start), _p(hist), _p(strand))
        if rc: self._err(rc)
        return hist[:nr], strand[:int(grp_off[-1])]

    # ---- include/ngsid_cigar.h
    def read_cigars(self, centres: ReadSet, rs: ReadSet, grp_off, read_order=None, k=13, w=20, clip=False, merge_m=False, cap=None):
        """ngsid_read_cigars: the alignment of every listed read to the centre of its group -> (aln [n_listed, 5] int32 in CIGAR_FIELDS order, op_off [n_listed + 1] uint64,
        ops uint32 = length << 4 | BAM op, strand [n_listed] int8).  ops[op_off[x]:op_off[x + 1]] are the ops of listed read x: soft clip, the runs of the counted columns
        ('=' 7, 'X' 8, 'I' 1, 'D' 2; merge_m: '=' and 'X' as 'M' 0), soft clip, in the oriented read's coordinates; a read without a strand or a counted column has none and
        -1 in its five fields.  Grouping, strands and counted columns as in consensus_support().  cap None: the count call, then the fill call (the store pass runs twice);
        a cap: the fill call alone (NgsidError NGSID_ERR_CAPACITY with .needed when there are more ops).  There is no CPU implementation: a library without the entry point
        is an error."""
        grp_off, ro, ng, strand, prm = self._support_head("read_cigars", "ngsid_cigar.h", ("read_cigars",), centres, grp_off, read_order, k, w, clip)
        nl = int(grp_off[-1])
        head = (C.byref(centres.c), C.byref(rs.c), _p(ro), _p(grp_off), C.c_uint64(ng), C.byref(prm), C.c_uint32(CIGAR_MERGE_M if merge_m else 0), _p(strand))
        (aln, op_off, ops), n = self._found_list("read_cigars", head, 3, lambda c: (np.full((max(nl, 1), CIGAR_NFIELD), -1, dtype=np.int32), np.zeros(nl + 1, dtype=np.uint64),
                                                                                   np.zeros(max(c, 1), dtype=np.uint32)), cap)
        return aln[:nl], op_off, ops[:n], strand[:nl]

    # ---- include/ngsid_errprof.h
    def error_profile(self, centres: ReadSet, rs: ReadSet, grp_off, read_order=None, k=13, w=20, clip=False, qualities=True):
        """ngsid_error_profile: what the reads of every group did to the letters of its centre, per strand -> (counts [n_groups, 2, ERRPROF_NCOUNT] uint64, qtab
        [n_groups, 2, ERRPROF_NQ, 3] uint64 or None, strand [n_listed] int8).  counts[g, s]: PAIR [4, 6] (centre letter x read letter A C G T, other, deleted), INS_LETTER [5],
        CEN_OTHER, READS, INS_LEN [16], DEL_LEN [16], HPCTX [8, 4] at the ERRPROF_* offsets; qtab[g, s, q]: read bases of reported quality q in '=', 'X' and 'I' columns
        (all zeros for a read set without qualities; qualities=False: None, the table and its cost are skipped).  Grouping, strands and counted columns as in
        consensus_support().  There is no CPU implementation: a library without the entry point is an error."""
        grp_off, ro, ng, strand, prm = self._support_head("error_profile", "ngsid_errprof.h", ("error_profile",), centres, grp_off, read_order, k, w, clip)
        counts = np.zeros((max(ng, 1), 2, ERRPROF_NCOUNT), dtype=np.uint64)
        qtab = np.zeros((max(ng, 1), 2, ERRPROF_NQ, 3), dtype=np.uint64) if qualities else None
        rc = self._call("error_profile", C.byref(centres.c), C.byref(rs.c), _p(ro), _p(grp_off), C.c_uint64(ng), C.byref(prm), _p(counts), _p(qtab), _p(strand))
        if rc: self._err(rc)
        return counts[:ng], None if qtab is None else qtab[:ng], strand[:int(grp_off[-1])]

    # ---- include/ngsid_phase.h
    def phase_genotypes(self, centres: ReadSet, rs: ReadSet, grp_off, site_off, site_pos, read_order=None, k=13, w=20, clip=False):
        """ngsid_phase_genotypes: the allele of every listed read at the sites site_pos[site_off[g]:site_off[g + 1]] (ascending centre positions, at most PHASE_MAX_SITES) of
        its group -> (geno uint8, geno_off [n_groups + 1], strand [n_listed] int8).  geno[geno_off[g]:geno_off[g + 1]].reshape(R_g, S_g) is group g, [listed read][site]:
        0-3 = A C G T, GENO_DEL, GENO_OTHER (mismatch with a read base outside ACGT), GENO_NONE (not counted).  Grouping, strands and counted columns as in consensus_support().
        There is no CPU implementation: a library without the entry point is an error."""
        grp_off, ro, ng, strand, prm = self._support_head("phase_genotypes", "ngsid_phase.h", ("phase_genotypes", "phase_pair_tables", "phase_assign"), centres, grp_off, read_order, k, w, clip)
        site_off = np.ascontiguousarray(site_off, dtype=np.uint64); site_pos = np.ascontiguousarray(site_pos, dtype=np.uint32)
        if len(site_off) != ng + 1 or len(site_pos) != int(site_off[-1]): raise ValueError("phase_genotypes: site_off has one entry per group + 1 and site_pos site_off[-1] entries")
        geno_off, _ = phase_offsets(grp_off, site_off)
        geno = np.full(max(int(geno_off[-1]), 1), GENO_NONE, dtype=np.uint8)
        rc = self._call("phase_genotypes", C.byref(centres.c), C.byref(rs.c), _p(ro), _p(grp_off), C.c_uint64(ng), C.byref(prm), _p(site_off), _p0(site_pos), _p(geno), _p(strand))
        if rc: self._err(rc)
        return geno[:int(geno_off[-1])], geno_off, strand[:int(grp_off[-1])]

    def phase_pair_tables(self, geno, grp_off, site_off):
        """ngsid_phase_pair_tables -> (tables uint32, tab_off [n_groups + 1]): tables[tab_off[g]:tab_off[g + 1]].reshape(S_g, S_g, 5, 5)[s, t, a, b], s < t, = listed reads of
        group g with code a at site s and code b at site t (both <= GENO_DEL); zero for s >= t."""
        self._need("ngsid_phase.h", "phase_genotypes", "phase_pair_tables", "phase_assign")
        grp_off = np.ascontiguousarray(grp_off, dtype=np.uint64); site_off = np.ascontiguousarray(site_off, dtype=np.uint64)
        geno_off, tab_off = phase_offsets(grp_off, site_off)
        geno = np.ascontiguousarray(geno, dtype=np.uint8)
        if len(geno) != int(geno_off[-1]): raise ValueError("phase_pair_tables: geno has %d entries, the offsets ask for %d" % (len(geno), int(geno_off[-1])))
        tables = np.zeros(max(int(tab_off[-1]), 1), dtype=np.uint32)
        rc = self._call("phase_pair_tables", _p0(geno), _p(grp_off), _p(site_off), C.c_uint64(len(grp_off) - 1), _p(tables))
        if rc: self._err(rc)
        return tables[:int(tab_off[-1])], tab_off

    def phase_assign(self, geno, grp_off, site_off, hap_off, hap_alleles):
        """ngsid_phase_assign: haplotypes hap_off[g]:hap_off[g + 1] (at most PHASE_MAX_HAPS) belong to group g, hap_alleles holds their [haplotype][site] blocks group after
        group (0 - GENO_DEL, or HAP_ANY) -> (best int8, dist uint8, dist2 uint8) per listed read: the nearest haplotype within the group (the lowest on ties), its distance
        over the sites both cover, and the smallest distance over the other haplotypes (255: none).  -1 / 255 / 255 for a read without a covered site or a group without haplotypes."""
        self._need("ngsid_phase.h", "phase_genotypes", "phase_pair_tables", "phase_assign")
        grp_off = np.ascontiguousarray(grp_off, dtype=np.uint64); site_off = np.ascontiguousarray(site_off, dtype=np.uint64); hap_off = np.ascontiguousarray(hap_off, dtype=np.uint64)
        geno_off, _ = phase_offsets(grp_off, site_off)
        geno = np.ascontiguousarray(geno, dtype=np.uint8); hal = np.ascontiguousarray(hap_alleles, dtype=np.uint8).ravel()
        need = int((np.diff(hap_off.astype(np.int64)) * np.diff(site_off.astype(np.int64))).sum())
        if len(geno) != int(geno_off[-1]) or len(hal) != need or len(hap_off) != len(grp_off): raise ValueError("phase_assign: geno / hap_alleles do not match the offsets")
        nl = int(grp_off[-1])
        best = np.full(max(nl, 1), -1, dtype=np.int8); dist = np.full(max(nl, 1), 255, dtype=np.uint8); dist2 = np.full(max(nl, 1), 255, dtype=np.uint8)
        rc = self._call("phase_assign", _p0(geno), _p(grp_off), _p(site_off), C.c_uint64(len(grp_off) - 1), _p(hap_off), _p0(hal),
                        _p(best), _p(dist), _p(dist2))
        if rc: self._err(rc)
        return best[:nl], dist[:nl], dist2[:nl]


    # ---- include/ngsid_demux.h
    def demux_locate(self, rs: ReadSet, tags, window=150, max_ed=3, iupac=True, matrices=False):
        """ngsid_demux_locate: every tag located in both end windows of every read -> hits [n, 2, 5] int32 in DEMUX_FIELDS order (side 1 in reverse-complement
        coordinates); matrices=True: (hits, ed_all [n, 2, T] int16, end_all [n, 2, T] int16), ed and end of every tag.  tags: a list of strings or a host ReadSet.
        There is no CPU implementation: a library without the entry point is an error."""
        self._need("ngsid_demux.h", "demux_locate")
        tg = _as_reads(tags)
        if tg.mem != MEM_HOST: raise ValueError("demux_locate takes the tags as a host read set")
        n, T = rs.n, tg.n
        hits = np.full((n, 2, 5), -1, dtype=np.int32)
        ed_all = np.full((n, 2, T), -1, dtype=np.int16) if matrices else None
        end_all = np.full((n, 2, T), -1, dtype=np.int16) if matrices else None
        prm = DemuxParams(int(window), int(max_ed), 1 if iupac else 0)
        rc = self._call("demux_locate", C.byref(rs.c), C.byref(tg.c), C.byref(prm), _p(hits), _p(ed_all), _p(end_all))
        if rc: self._err(rc)
        return (hits, ed_all, end_all) if matrices else hits

    def demux_scan(self, rs: ReadSet, patterns, max_ed=3, iupac=True, cap=None):
        """ngsid_demux_scan: every place in the whole read where a pattern occurs within max_ed edits, one hit per run of qualifying positions -> (hit_off [n + 1]
        uint64, hits [H, 3] int32 in DEMUX_SCAN_FIELDS order), within a read in ascending (end, pattern) order.  The count call (cap = 0), then the fill call; cap: one
        call with room for that many hits (NgsidError NGSID_ERR_CAPACITY with .needed when there are more).  patterns: a list of strings or a host ReadSet; reverse
        complements are patterns of their own.  There is no CPU implementation: a library without the entry point is an error."""
        self._need("ngsid_demux.h", "demux_scan")
        pt = _as_reads(patterns)
        if pt.mem != MEM_HOST: raise ValueError("demux_scan takes the patterns as a host read set")
        prm = DemuxScanParams(int(max_ed), 1 if iupac else 0)
        (hit_off, hits), n = self._found_list("demux_scan", (C.byref(rs.c), C.byref(pt.c), C.byref(prm)), 2,
                                              lambda c: (np.zeros(rs.n + 1, dtype=np.uint64), np.zeros((max(c, 1), 3), dtype=np.int32)), cap)
        return hit_off, hits[:n]

    # ---- include/ngsid_classify.h
    def refdb_build(self, refs, k=13, w=20) -> "RefDb":
        """ngsid_refdb_build: the minimizer index of a reference library (a list of strings or a host ReadSet) on the device -> RefDb handle (.info(), .release(),
        context manager).  There is no CPU implementation: a library without the entry point is an error."""
        self._need("ngsid_classify.h", "refdb_build", "classify_search")
        rs = _as_reads(refs)
        if rs.mem != MEM_HOST: raise ValueError("refdb_build takes the references as a host read set")
        prm = RefDbParams(int(k), int(w)); h = C.c_void_p()
        rc = self._call("refdb_build", C.byref(rs.c), C.byref(prm), C.byref(h))
        if rc: self._err(rc)
        return RefDb(self, h, int(k), int(w), rs)

    def classify_search(self, refdb: "RefDb", queries: ReadSet, top_k=8, min_shared=3, n_codes=False):
        """ngsid_classify_search -> (cand_ref [n, top_k] int32, cand_shared [n, top_k] int32, cand_strand [n, top_k] int8), -1 where a query has fewer candidates;
        n_codes=True: + n_codes [n, 2] int32, the distinct minimizer codes of each query strand."""
        self._need("ngsid_classify.h", "refdb_build", "classify_search")
        if refdb.api is not self or refdb.handle is None: raise NgsidError(-2, "the reference library was released or belongs to another context")
        n = queries.n; K = max(int(top_k), 0)
        ref = np.full((n, K), -1, dtype=np.int32); sh = np.full((n, K), -1, dtype=np.int32); st = np.full((n, K), -1, dtype=np.int8)
        nc = np.zeros((n, 2), dtype=np.int32) if n_codes else None
        prm = ClassifyParams(int(top_k), int(min_shared))
        rc = self._call("classify_search", refdb.handle, C.byref(queries.c), C.byref(prm), _p(ref), _p(sh), _p(st), _p(nc))
        if rc: self._err(rc)
        return (ref, sh, st, nc) if n_codes else (ref, sh, st)

    # ---- include/ngsid_chimera.h
    def chimera_model(self, queries, parents, pair_off, pair_parent, pair_gid=None, profiles=False):
        """ngsid_chimera_model: the best one-parent and two-parent model of every query over its pairs pair_parent[pair_off[q]:pair_off[q + 1]] (indices into parents;
        pair_gid: pairs of one gid are never combined, None = the parent index) -> fields [n, 7] int32 in CHIMERA_FIELDS order, -1 where a model does not exist;
        profiles=True: (fields, prof uint16, prof_off [n_pairs + 1]): prof[prof_off[k]:prof_off[k + 1]] = F_k[0 .. n] then B_k[0 .. n] of pair k.  queries / parents: lists of
        strings or read sets; the pair arrays are host arrays.  There is no CPU implementation: a library without the entry point is an error."""
        self._need("ngsid_chimera.h", "chimera_model")
        qs, ps = _as_reads(queries), _as_reads(parents)
        po = np.ascontiguousarray(pair_off, dtype=np.uint64)
        pp = np.ascontiguousarray(pair_parent, dtype=np.uint32)
        pg = None if pair_gid is None else np.ascontiguousarray(pair_gid, dtype=np.int32)
        if len(po) != qs.n + 1: raise ValueError("chimera_model: pair_off has one entry per query + 1")
        if len(pp) != int(po[-1]) or (pg is not None and len(pg) != len(pp)): raise ValueError("chimera_model: pair_parent / pair_gid hold pair_off[-1] entries")
        fields = np.full((qs.n, CHIMERA_NFIELD), -1, dtype=np.int32)
        prof = prof_off = None
        if profiles:
            if qs.mem != MEM_HOST: raise ValueError("chimera_model: profiles=True takes the queries as a host read set (their lengths size the result)")
            prof_off = chimera_profile_offsets(np.diff(qs.off.astype(np.int64)), po)
            prof = np.zeros(max(int(prof_off[-1]), 1), dtype=np.uint16)
        rc = self._call("chimera_model", C.byref(qs.c), C.byref(ps.c), _p(po), _p0(pp), _p0(pg), _p0(fields), _p(prof))
        if rc: self._err(rc)
        return (fields, prof[:int(prof_off[-1])], prof_off) if profiles else fields

    # ---- include/ngsid_near.h
    def ed_within(self, queries, targets, q_idx, t_idx, max_dist, both_strands=True):
        """ngsid_ed_within_batch: for the listed pairs the unit-cost edit distance of queries[q_idx[p]] and targets[t_idx[p]], over both strands with both_strands
        (the smaller one; a tie goes to forward) -> (dist int32 [n], strand uint8 [n]): dist = -1 and strand = 0 where the distance exceeds max_dist (0 .. NEAR_MAX_DIST).
        queries / targets: lists of strings or read sets.  There is no CPU implementation: a library without the entry point is an error."""
        self._need("ngsid_near.h", "ed_within_batch", "near_pairs")
        return self._ed_within("ed_within_batch", queries, targets, q_idx, t_idx, max_dist, both_strands)

    def ed_within_wide(self, queries, targets, q_idx, t_idx, max_dist, both_strands=True):
        """ngsid_ed_within_wide_batch: ed_within with max_dist 0 .. NEAR_WIDE_MAX_DIST (a band of 2, 4 or 8 words per lane above NEAR_MAX_DIST, the one-word kernel
        below); the same arguments, dtypes and shapes.  There is no CPU implementation: a library without the entry point is an error."""
        self._need("ngsid_near.h", "ed_within_wide_batch", "near_pairs_wide")
        return self._ed_within("ed_within_wide_batch", queries, targets, q_idx, t_idx, max_dist, both_strands)

    def _ed_within(self, entry, queries, targets, q_idx, t_idx, max_dist, both_strands):
        qs, ts = _as_reads(queries), _as_reads(targets)
        qi = np.ascontiguousarray(q_idx, dtype=np.uint32); ti = np.ascontiguousarray(t_idx, dtype=np.uint32)
        if len(qi) != len(ti): raise ValueError("ed_within: q_idx and t_idx hold one entry per pair")
        n = len(qi)
        dist = np.full(max(n, 1), -1, dtype=np.int32); strand = np.zeros(max(n, 1), dtype=np.uint8)
        rc = self._call(entry, C.byref(qs.c), C.byref(ts.c), _p0(qi), _p0(ti), C.c_uint64(n),
                        C.c_int32(int(max_dist)), C.c_uint32(NEAR_BOTH_STRANDS if both_strands else 0), _p(dist), _p(strand))
        if rc: self._err(rc)
        return dist[:n], strand[:n]

    def near_pairs(self, seqs, max_dist, both_strands=True, cap=None):
        """ngsid_near_pairs: every pair i < j of seqs within max_dist edits (0 .. NEAR_MAX_DIST; both strands with both_strands) -> (pair_i uint32, pair_j uint32,
        dist uint8, strand uint8), in ascending (i, j) order.  The count call (cap = 0), then the fill call; cap: one call with room for that many pairs
        (NgsidError NGSID_ERR_CAPACITY with .needed when there are more).  There is no CPU implementation: a library without the entry point is an error."""
        self._need("ngsid_near.h", "ed_within_batch", "near_pairs")
        return self._near_pairs("near_pairs", seqs, max_dist, both_strands, cap)

    def near_pairs_wide(self, seqs, max_dist, both_strands=True, cap=None):
        """ngsid_near_pairs_wide: near_pairs with max_dist 0 .. NEAR_WIDE_MAX_DIST; the same arguments, dtypes (dist stays uint8: 255 fits) and shapes.  There is no
        CPU implementation: a library without the entry point is an error."""
        self._need("ngsid_near.h", "ed_within_wide_batch", "near_pairs_wide")
        return self._near_pairs("near_pairs_wide", seqs, max_dist, both_strands, cap)

    def _near_pairs(self, entry, seqs, max_dist, both_strands, cap):
        rs = _as_reads(seqs)
        found = C.c_uint64(0)
        outs, _ = self._found_list(entry, (C.byref(rs.c), C.c_int32(int(max_dist)), C.c_uint32(NEAR_BOTH_STRANDS if both_strands else 0)), 4,
                                   lambda c: tuple(np.zeros(max(c, 1), dtype=t) for t in (np.uint32, np.uint32, np.uint8, np.uint8)), cap, tail=(C.byref(found),))
        return tuple(a[:int(found.value)] for a in outs)

    # ---- include/ngsid_umi.h
    def umi_pairs(self, seqs, max_dist, seed_len, cap=None):
        """ngsid_umi_pairs: every pair i < j of seqs (at most UMI_MAX_LEN letters each) within max_dist edits (0 .. UMI_MAX_DIST), found by the seeded search ->
        (pair_i uint32, pair_j uint32, dist uint8), in ascending (i, j) order: what near_pairs(seqs, max_dist, both_strands=False) returns without its strand array,
        whatever seed_len (4 .. 16) is.  The count call (cap = 0), then the fill call; cap: one call with room for that many pairs (NgsidError NGSID_ERR_CAPACITY with
        .needed when there are more).  There is no CPU implementation: a library without the entry point is an error."""
        self._need("ngsid_umi.h", "umi_pairs", "umi_centroids")
        rs = _as_reads(seqs)
        prm = UmiParams(int(max_dist), int(seed_len))
        found = C.c_uint64(0)
        outs, _ = self._found_list("umi_pairs", (C.byref(rs.c), C.byref(prm)), 3, lambda c: tuple(np.zeros(max(c, 1), dtype=t) for t in (np.uint32, np.uint32, np.uint8)), cap, tail=(C.byref(found),))
        return tuple(a[:int(found.value)] for a in outs)

    def umi_centroids(self, pair_i, pair_j, order):
        """ngsid_umi_centroids (a host function): the nodes 0 .. len(order) - 1 walked in `order`, each joining the earliest-founded centroid it shares a listed pair
        with or founding a bin -> (bin_of int32 [n], centroid uint32 [n_bins] in founding order)"""
        self._need("ngsid_umi.h", "umi_pairs", "umi_centroids")
        pi = np.ascontiguousarray(pair_i, dtype=np.uint32); pj = np.ascontiguousarray(pair_j, dtype=np.uint32); od = np.ascontiguousarray(order, dtype=np.uint32)
        if len(pi) != len(pj): raise ValueError("umi_centroids: pair_i and pair_j hold one entry per pair")
        n = len(od)
        bin_of = np.full(max(n, 1), -1, dtype=np.int32); cent = np.zeros(max(n, 1), dtype=np.uint32); nb = C.c_uint32(0)
        f = self._fn("umi_centroids")
        rc = f(_p0(pi), _p0(pj), C.c_uint64(len(pi)), _p0(od), C.c_uint32(n),
               _p(bin_of), _p(cent), C.byref(nb))
        if rc: raise NgsidError(rc, "umi_centroids: an index out of range, a pair (x, x), or an order that is no permutation")
        return bin_of[:n], cent[:int(nb.value)].copy()

    # ---- include/ngsid_recruit.h
    def recruit(self, rs: ReadSet, read_off, cons, cons_off, max_ed, both_strands=True):
        """ngsid_recruit: every read located inside every consensus of its group (reads read_off[g]:read_off[g + 1] against consensuses cons_off[g]:cons_off[g + 1]),
        on both strands with both_strands, and the two nearest consensuses per read -> hits [n, 6] int32 in RECRUIT_FIELDS order: -1 where there is nothing, strand 0.
        max_ed: one bound per consensus.  cons: a list of strings or a host ReadSet.  There is no CPU implementation: a library without the entry point is an error."""
        self._need("ngsid_recruit.h", "recruit")
        cs = _as_reads(cons)
        if cs.mem != MEM_HOST: raise ValueError("recruit takes the consensuses as a host read set")
        ro = np.ascontiguousarray(read_off, dtype=np.uint64); co = np.ascontiguousarray(cons_off, dtype=np.uint64)
        me = np.ascontiguousarray(max_ed, dtype=np.int32)
        if len(ro) != len(co) or len(ro) < 1: raise ValueError("recruit: read_off and cons_off hold one entry per group + 1")
        if len(me) != cs.n: raise ValueError("recruit: max_ed holds one entry per consensus")
        hits = np.full((max(rs.n, 1), RECRUIT_NFIELD), -1, dtype=np.int32); hits[:, 2] = 0
        rc = self._call("recruit", C.byref(rs.c), _p(ro), C.byref(cs.c), _p(co), C.c_uint64(len(ro) - 1), _p0(me), C.c_uint32(RECRUIT_BOTH_STRANDS if both_strands else 0), _p(hits))
        if rc: self._err(rc)
        return hits[:rs.n]


class RefDb:
    """handle of a reference library built by Api.refdb_build; owned by that context (released with it at the latest)"""

    def __init__(self, api, handle, k, w, refs=None):
        self.api, self.handle, self.k, self.w = api, handle, k, w
        self.refs = refs          # the host read set it was built from: classify.verify aligns against it

    def info(self):
        """-> dict(n_refs, n_postings, n_codes, device_bytes)"""
        if self.handle is None: raise NgsidError(-2, "the reference library was released")
        v = [C.c_uint64(0) for _ in range(4)]
        f = self.api._fn("refdb_info")
        rc = f(self.handle, *[C.byref(x) for x in v])
        if rc: self.api._err(rc)
        return dict(zip(("n_refs", "n_postings", "n_codes", "device_bytes"), (int(x.value) for x in v)))

    def release(self):
        """idempotent"""
        h, self.handle = self.handle, None
        if h is not None and self.api.ctx is not None:
            rc = self.api._call("refdb_release", h)
            if rc: self.api._err(rc)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()
        return False
