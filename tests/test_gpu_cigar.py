"""GPU: ngsid_read_cigars (include/ngsid_cigar.h) through the C-ABI == the definition restated from the oracle's parts (tests/cigar_reference.py), exactly - aln, op_off,
ops and strand -, hand cases against literal CIGAR strings, the support counters recomputed from the CIGARs, and the pipeline / SAM / CLI layers on top of it."""
import os
import numpy as np
import pytest
from oracle_lib import GOLD
from ngspeciesid_amd import synth, pipeline, fastio, sam
from ngspeciesid_amd._capi import ReadSet, NgsidError
from ngspeciesid_amd.hostutil import subset_reads
from ngspeciesid_amd.ptable import select_p_table
from support_reference import _COMP
from cigar_reference import cigar_reference, walk_record, oriented

pytestmark = pytest.mark.gpu


def _rs(rd):
    return ReadSet(rd["seq"].numpy(), rd["qual"].numpy(), rd["off"].numpy().astype(np.uint64))


def _rc(s):
    return _COMP[np.frombuffer(s.encode(), dtype=np.uint8)[::-1]].tobytes().decode()


def _same(api, oracle, centres, rs, grp_off, read_order=None, k=13, w=20, clip=False, merge_m=False, what="", only=None, got=None):
    grp_off = np.asarray(grp_off, dtype=np.uint64)
    if got is None: got = api.read_cigars(ReadSet.from_strings(centres), rs, grp_off, read_order=read_order, k=k, w=w, clip=clip, merge_m=merge_m)
    exp = cigar_reference(oracle, centres, rs, grp_off, read_order, k, w, clip, merge_m, only=only)
    assert np.array_equal(got[3], exp[3]), what + ": strand"
    if only is None:
        assert np.array_equal(got[1], exp[1]), what + ": op_off"
        bad = np.nonzero((got[0] != exp[0]).any(axis=1))[0]
        assert len(bad) == 0, "%s: %d aln rows differ, first %d: HIP %s reference %s" % (what, len(bad), bad[0], got[0][bad[0]].tolist(), exp[0][bad[0]].tolist())
        assert np.array_equal(got[2], exp[2]), what + ": ops"
    else:
        cg, ce = sam.cigar_strings(got[1], got[2]), sam.cigar_strings(exp[1], exp[2])
        for x in sorted(only):
            assert got[0][x].tolist() == exp[0][x].tolist() and cg[x] == ce[x], "%s: listed read %d" % (what, x)
    assert got[0].dtype == np.int32 and got[1].dtype == np.uint64 and got[2].dtype == np.uint32 and got[3].dtype == np.int8
    return got


def _mutate(rng, s, n_sub=0, n_del=0, n_ins=0):
    a = list(s)
    for _ in range(n_sub):
        i = int(rng.integers(len(a))); a[i] = "ACGT"[("ACGT".index(a[i]) + 1 + int(rng.integers(3))) % 4]
    for _ in range(n_del):
        del a[int(rng.integers(len(a)))]
    for _ in range(n_ins):
        a.insert(int(rng.integers(len(a) + 1)), "ACGT"[int(rng.integers(4))])
    return "".join(a)


# a 130-letter centre without a repeat at the places the hand cases edit: every case has ONE minimum-cost alignment
HAND_CENTRE = ("ACGTTGCATCAGGCTTACGATCGGATACCTGAGTCATGCCATAGCTAGGTCCATGATCGTTACGGCATTAG" "CATGGACTTCAGTACGCTAGTTCGAACTGGTCATCGGTACCTAGGATCGCTTAACGGTCA")[:130]
HAND_OTHER = "TGCAGGTACCATGCTTAGCAATCGGACTTGCAGTACCGTTAGCATCGGAATCCGTAGCTTAGGCATCAAGTCGGCATTACG"


def _hand():
    c = HAND_CENTRE
    assert len(c) == 130
    z = [l for l in "ACGT" if l != c[-1]]
    over = "GGTTGGTTAACC" + c + (z[0] + z[1]) * 6                  # (the centre's last letter does not occur behind it: the traceback, diagonal first, cannot match it further right)
    ins = "ACGT"[[x for x in range(4) if "ACGT"[x] not in (c[63], c[64])][0]]
    reads = [c,                                   # 0: equal to its centre
             c[30:110],                           # 1: an interior piece
             over,                                # 2: overhangs on both ends
             c[:64] + ins + c[64:],               # 3: one inserted base behind position 63
             c[:62] + c[65:],                     # 4: positions 62 - 64 deleted
             c[:40] + "N" + c[41:],               # 5: an N
             _rc(over),                           # 6: the reverse complement of 2
             "AG" * 60,                           # 7: shares no minimizer
             HAND_OTHER]                          # 8: the one read of the last group
    centres = [c, HAND_OTHER, HAND_OTHER]
    grp_off = np.array([0, 8, 8, 9], dtype=np.uint64)                          # group 1 is empty, group 2 has one read
    cig = ["130=", "80=", "12S130=12S", "64=1I66=", "62=3D65=", "40=1X89=", "12S130=12S", "*", "%d=" % len(HAND_OTHER)]
    aln = [[0, 129, 0, 129, 0], [30, 109, 0, 79, 0], [0, 129, 12, 141, 0], [0, 129, 0, 130, 1], [0, 129, 0, 126, 3], [0, 129, 0, 129, 1], [0, 129, 12, 141, 0], [-1] * 5,
           [0, len(HAND_OTHER) - 1, 0, len(HAND_OTHER) - 1, 0]]
    return centres, reads, grp_off, cig, aln, [0, 0, 0, 0, 0, 0, 1, -1, 0]


def test_hand_cases(gpu_api, oracle):
    centres, reads, grp_off, cig, aln, strand = _hand()
    rs = ReadSet.from_strings(reads)
    got = _same(gpu_api, oracle, centres, rs, grp_off, what="hand cases")
    assert sam.cigar_strings(got[1], got[2]) == cig and got[0].tolist() == aln and got[3].tolist() == strand
    m = _same(gpu_api, oracle, centres, rs, grp_off, merge_m=True, what="hand cases, merge_m")
    assert sam.cigar_strings(m[1], m[2]) == [c.replace("=", "M") for c in cig[:5]] + ["130M"] + [c.replace("=", "M") for c in cig[6:]]
    assert np.array_equal(m[0], got[0]) and np.array_equal(m[3], got[3])
    # nothing listed at all, no reads at all, a centre of length 0
    z = gpu_api.read_cigars(ReadSet.from_strings(centres), rs, np.zeros(4, dtype=np.uint64))
    assert z[0].shape == (0, 5) and z[1].tolist() == [0] and len(z[2]) == 0 and len(z[3]) == 0
    z = gpu_api.read_cigars(ReadSet.from_strings(centres), ReadSet.from_strings([]), np.zeros(4, dtype=np.uint64))
    assert z[0].shape == (0, 5) and z[1].tolist() == [0] and len(z[2]) == 0
    z = gpu_api.read_cigars(ReadSet.from_strings(["", centres[0]]), rs, np.array([0, 2, 3], dtype=np.uint64))
    assert z[0][:2].tolist() == [[-1] * 5] * 2 and sam.cigar_strings(z[1], z[2]) == ["*", "*", "12S130=12S"]


def test_centre_lengths_across_steps(gpu_api, oracle):
    """centres of 8, 63, 64, 65, 129 and 520 letters, 30 reads each at 10 % error, in one call"""
    rng = np.random.default_rng(17)
    centres, reads, off = [], [], [0]
    for L in (8, 63, 64, 65, 129, 520):
        c = synth.make_species(1, max(L, 40), 0.0, seed=300 + L)[0].tobytes().decode()[:L]
        centres.append(c)
        for x in range(30):
            e = max(1, L // 30)
            r = _mutate(rng, c, n_sub=e, n_del=e, n_ins=e) if x % 5 else c
            if x % 3 == 0: r = "GATTACA"[:x % 7] + r + "CCTGA"[:x % 5]
            if x % 7 == 3 and len(r) > 20: r = r[5:-4]
            reads.append(_rc(r) if x % 2 else r)
        off.append(len(reads))
    got = _same(gpu_api, oracle, centres, ReadSet.from_strings(reads), np.array(off, dtype=np.uint64), what="centre lengths")
    per = np.add.reduceat((got[0][:, 0] >= 0).astype(int), off[:-1])
    assert (per[1:] >= 25).all()                                                   # (a centre of 8 letters holds no 13-mer: no strand, no ops)


@pytest.mark.parametrize("clip", [False, True])
def test_random_groups(gpu_api, oracle, clip):
    """3 groups x 200 reads of about 300 letters at 5 % and 15 % error, both strands, read_order permuted"""
    sp = synth.make_species(3, 300, 0.2, seed=91)
    rd = [synth.make_reads(sp, 400, mu=mu, seed=92 + i, rc_fraction=0.5) for i, mu in enumerate((13.0, 8.2))]      # mean Phred 13 ~ 5 %, 8.2 ~ 15 %
    parts = [_rs(r) for r in rd]
    species = np.concatenate([r["species"].numpy() for r in rd])
    seq = np.concatenate([p.seq for p in parts]); lens = np.concatenate([np.diff(p.off.astype(np.int64)) for p in parts])
    o = np.zeros(len(lens) + 1, dtype=np.uint64); o[1:] = np.cumsum(lens)
    rs = ReadSet(seq, None, o)
    rng = np.random.default_rng(3)
    lists = [rng.permutation(np.nonzero(species == g)[0])[:200].astype(np.uint32) for g in range(3)]
    assert all(len(l) == 200 for l in lists)
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
    got = _same(gpu_api, oracle, [s.tobytes().decode() for s in sp], rs, off, np.concatenate(lists), clip=clip, what="random groups, clip %d" % clip)
    assert (got[3] == 1).sum() > 150 and (got[3] == 0).sum() > 150 and (got[0][:, 4] > 20).sum() > 100


def _chunk_case():
    rng = np.random.default_rng(23)
    c = synth.make_species(1, 2000, 0.0, seed=95)[0].tobytes().decode()
    reads = []
    for x in range(700):
        a = int(rng.integers(0, 1880)); r = _mutate(rng, c[a:a + 120], n_sub=4, n_del=2, n_ins=2)
        reads.append(_rc(r) if x % 2 else r)
    return c, ReadSet.from_strings(reads)


def test_chunks_of_the_path_matrix(gpu_api, oracle):
    """one 2 000-letter centre, 700 reads of 120 letters, a budget of 1 MB: a row is 256 dwords x 20 bytes = 5 120 bytes, 204 rows a chunk, at least three chunks"""
    c, rs = _chunk_case()
    off = np.array([0, 700], dtype=np.uint64)
    whole = gpu_api.read_cigars(ReadSet.from_strings([c]), rs, off)
    assert ((1 << 20) // (((2000 + 63) & ~63) // 8 * 20)) * 3 < 700
    gpu_api.set_option("support_budget_mb", 1)
    try:
        parts = gpu_api.read_cigars(ReadSet.from_strings([c]), rs, off)
    finally:
        gpu_api.set_option("support_budget_mb", 0)
    assert all(np.array_equal(x, y) for x, y in zip(whole, parts))
    assert (whole[0][:, 0] >= 0).sum() > 650
    _same(gpu_api, oracle, [c], rs, off, what="chunks", only=set(range(0, 700, 7)), got=parts)


def test_capacity_protocol(gpu_api, oracle):
    centres, reads, grp_off, cig, _, _ = _hand()
    rs = ReadSet.from_strings(reads); cs = ReadSet.from_strings(centres)
    exp = cigar_reference(oracle, centres, rs, grp_off)
    needed = len(exp[2])
    assert needed == sum(len(sam.cigar_ops(c)) for c in cig)
    with pytest.raises(NgsidError) as e:
        gpu_api.read_cigars(cs, rs, grp_off, cap=needed - 1)
    assert e.value.code == -4 and e.value.needed == needed
    got = gpu_api.read_cigars(cs, rs, grp_off, cap=needed)
    assert np.array_equal(got[2], exp[2]) and np.array_equal(got[1], exp[1])
    more = gpu_api.read_cigars(cs, rs, grp_off, cap=needed + 100)
    assert all(np.array_equal(x, y) for x, y in zip(got, more))
    # the count call alone, through the raw entry point: needed, NGSID_ERR_CAPACITY
    import ctypes as C
    from ngspeciesid_amd._capi import SupportParams, _p
    n = C.c_uint64(0); prm = SupportParams(13, 20, 0)
    rc = gpu_api._call("read_cigars", C.byref(cs.c), C.byref(rs.c), None, _p(grp_off), C.c_uint64(3), C.byref(prm), C.c_uint32(0), None, None, None, None, C.c_uint64(0), C.byref(n))
    assert rc == -4 and n.value == needed
    rc = gpu_api._call("read_cigars", C.byref(cs.c), C.byref(rs.c), None, _p(grp_off), C.c_uint64(3), C.byref(prm), C.c_uint32(2), None, None, None, None, C.c_uint64(0), C.byref(n))
    assert rc == -2                                                                # an unknown flag


def test_support_counters_from_the_cigars(gpu_api):
    """independent of the oracle: depth, agree, A / C / G / T, del and ins_after recomputed from the returned CIGARs and the oriented reads == Api.consensus_support"""
    sp = synth.make_species(2, 400, 0.2, seed=97)
    rd = synth.make_reads(sp, 500, mu=11.0, seed=98, rc_fraction=0.5)
    rs = _rs(rd); species = rd["species"].numpy()
    lists = [np.nonzero(species == g)[0].astype(np.uint32) for g in range(2)]
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64); ro = np.concatenate(lists)
    centres = [s.tobytes().decode() for s in sp]
    for clip in (False, True):
        counts, cen_off, used, strand = gpu_api.consensus_support(ReadSet.from_strings(centres), rs, off, read_order=ro, clip=clip)
        aln, op_off, ops, strand2 = gpu_api.read_cigars(ReadSet.from_strings(centres), rs, off, read_order=ro, clip=clip)
        assert np.array_equal(strand, strand2)
        mine = np.zeros_like(counts); n_used = np.zeros(2, dtype=np.uint64)
        for g in range(2):
            cnt = mine[int(cen_off[g]):int(cen_off[g + 1])]
            for x in range(int(off[g]), int(off[g + 1])):
                if aln[x, 0] < 0: continue
                n_used[g] += 1
                read = oriented(rs, int(ro[x]), int(strand[x])); qi, ti = 0, int(aln[x, 0])
                for v in ops[int(op_off[x]):int(op_off[x + 1])].tolist():
                    n, op = v >> 4, v & 15
                    if op == 7: cnt[ti:ti + n, 0] += 1; cnt[ti:ti + n, 1] += 1
                    elif op == 8:
                        cnt[ti:ti + n, 0] += 1
                        for d in range(n):
                            k = "ACGT".find(chr(int(read[qi + d]) & 0xDF))
                            if k >= 0: cnt[ti + d, 2 + k] += 1
                    elif op == 2: cnt[ti:ti + n, 0] += 1; cnt[ti:ti + n, 6] += 1
                    elif op == 1: cnt[ti - 1, 7] += 1
                    if op in (7, 8, 1, 4): qi += n
                    if op in (7, 8, 2): ti += n
                assert qi == len(read) and ti == int(aln[x, 1]) + 1
        assert np.array_equal(n_used, used) and np.array_equal(mine, counts) and counts[:, 7].sum() > 100 and counts[:, 6].sum() > 100


def _sample_h1(api):
    rd = fastio.read_fastq(os.path.join(GOLD, "sample_h1.fastq"))
    rs = rd[1] if isinstance(rd, tuple) else rd
    score, err, keep = api.score_reads(rs, 13, 7.0)
    idx = np.nonzero(keep)[0]; idx = idx[np.argsort(-score[idx], kind="stable")]
    return subset_reads(rs, idx), score[idx]


KW = dict(k=13, w=20, abundance_ratio=0.05, racon_iter=2, band=0, p_shared=select_p_table(13, 20))


def test_pipeline_key(gpu_api, oracle):
    sub, score = _sample_h1(gpu_api)
    kw = dict(KW, acc_rank=np.arange(sub.n, dtype=np.uint32))
    a = pipeline.run_hot_path(gpu_api, sub, score, **kw)
    b = pipeline.run_hot_path(gpu_api, sub, score, alignments=True, **kw)
    assert sorted(b) == sorted(list(a) + ["alignments"]) and a["centers"] == b["centers"]
    for key in a:
        if key != "centers": assert np.array_equal(a[key], b[key]), key
    lists = [np.concatenate([np.nonzero(b["rep_of"] == r)[0] for r in c[4]]).astype(np.uint32) for c in b["centers"]]      # the pooled lists
    centres = [c[3] for c in b["centers"]]
    assert centres and len(b["alignments"]) == len(centres)
    for e, l in zip(b["alignments"], lists):
        assert np.array_equal(e["reads"], l) and len(e["aln"]) == len(l) == len(e["strand"]) == len(e["op_off"]) - 1 and int(e["op_off"][0]) == 0 and int(e["op_off"][-1]) == len(e["ops"])
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
    got = _same(gpu_api, oracle, centres, sub, off, np.concatenate(lists), what="sample_h1")
    assert np.array_equal(np.concatenate([e["aln"] for e in b["alignments"]]), got[0]) and np.array_equal(np.concatenate([e["ops"] for e in b["alignments"]]), got[2])
    assert (got[0][:, 0] >= 0).sum() > 200
    # many samples in one pass: the key of every sample is what the sample gets alone
    seg = np.array([0, sub.n], dtype=np.uint64)
    many = pipeline.run_hot_path_samples(gpu_api, sub, score, seg, alignments=True, **kw)
    assert len(many) == 1 and len(many[0]["alignments"]) == len(b["alignments"])
    for x, y in zip(many[0]["alignments"], b["alignments"]):
        assert all(np.array_equal(x[f], y[f]) for f in ("reads", "strand", "aln", "op_off", "ops"))


def _files(out):
    res = {}
    for root, _, fs in os.walk(out):
        for f in fs:
            res[os.path.relpath(os.path.join(root, f), out)] = open(os.path.join(root, f), "rb").read()
    return res


def _check_sam_file(path, fasta_text, n_min):
    head, seq = fasta_text.decode().split("\n")[:2]
    p = sam.parse_sam(path)
    assert p["targets"] == [(head[1:].split()[0], len(seq))] and p["header"][0].startswith("@HD") and p["header"][-1].startswith("@PG")
    mapped = p["flag"] != 4
    assert mapped.sum() >= n_min and set(p["flag"].tolist()) <= {0, 4, 16}
    for x in np.nonzero(mapped)[0]:
        ops = sam.cigar_ops(p["cigar"][x])
        assert p["rname"][x] == p["targets"][0][0] and p["mapq"][x] == 255 and len(p["seq"][x]) == len(p["qual"][x])
        nm, _ = walk_record(ops, p["seq"][x], seq, int(p["pos"][x]))
        assert nm == p["nm"][x]
    for x in np.nonzero(~mapped)[0]:
        assert (p["rname"][x], p["pos"][x], p["cigar"][x]) == ("*", 0, "*")
    return p


def test_cli_flag_and_sub_command(gpu_api, tmp_path):
    from ngspeciesid_amd import cli as _cli, fastpath, recruit
    res = []
    for flag in ([], ["--write_sam"]):
        out = str(tmp_path / ("o%d" % len(flag))); os.makedirs(out)
        args = _cli.build_parser().parse_args(["--ont", "--fastq", os.path.join(GOLD, "sample_h1.fastq"), "--outfolder", out, "--t", "1", "--consensus", "--racon", "--racon_iter", "2"] + flag); args.k, args.w = 13, 20
        r = fastpath.main(args, api=gpu_api)
        res.append(_files(out))
    a, b = res
    stems = sorted(f[:-len("consensus.fasta")] for f in a if f.endswith(os.sep + "consensus.fasta"))
    assert stems and sorted(set(b) - set(a)) == sorted(s + "reads_to_consensus.sam" for s in stems)
    assert all(a[f] == b[f] for f in a if f != "logfile.txt")
    out = str(tmp_path / "o1")
    for s in stems:
        p = _check_sam_file(os.path.join(out, s + "reads_to_consensus.sam"), b[s + "consensus.fasta"], 20)
        assert any("I" in c for c in p["cigar"]) and any("D" in c for c in p["cigar"]) and not any("M" in c for c in p["cigar"])
    # without --racon, with 'M'
    out2 = str(tmp_path / "o2"); os.makedirs(out2)
    args = _cli.build_parser().parse_args(["--ont", "--fastq", os.path.join(GOLD, "sample_h1.fastq"), "--outfolder", out2, "--t", "1", "--consensus", "--write_sam", "--sam_merge_m"]); args.k, args.w = 13, 20
    fastpath.main(args, api=gpu_api)
    c = _files(out2)
    sams = sorted(f for f in c if f.endswith(".sam"))
    assert sams and sams == sorted(f[:-len(".fasta")] + ".sam" for f in c if f.startswith("consensus_reference_") and f.endswith(".fasta"))
    for f in sams:
        p = _check_sam_file(os.path.join(out2, f), c[f[:-len(".sam")] + ".fasta"], 20)
        assert not any("=" in x or "X" in x for x in p["cigar"])
    # the sub-command: the sorted reads against the consensuses the run wrote - its mapped reads are those recruit assigns
    fa = str(tmp_path / "cons.fasta")
    with open(fa, "w") as f:
        for s in stems: f.write(b[s + "consensus.fasta"].decode())
    sq = os.path.join(out, "sorted.fastq")
    sargs = _cli._sam_subparser(__import__("argparse").ArgumentParser()).parse_args(["--fastq", sq, "--fasta", fa, "--outfile", str(tmp_path / "all.sam")])
    sub = sam.sam_fastq(sargs, api=gpu_api)
    p = sam.parse_sam(str(tmp_path / "all.sam"))
    rargs = _cli._recruit_subparser(__import__("argparse").ArgumentParser()).parse_args(["--fastq", sq, "--fasta", fa, "--outfolder", str(tmp_path / "rec")])
    rec = recruit.recruit_fastq(rargs, api=gpu_api)
    asg = [l.split("\t") for l in open(str(tmp_path / "rec" / "read_assignments.tsv")).read().splitlines()][1:]
    assert len(p["targets"]) == len(stems) and len(p["qname"]) == len(asg) == sub["records"]
    want = {x[0]: x[1] for x in asg if x[5] == "assigned"}
    have = {q: t for q, t, fl in zip(p["qname"].tolist(), p["rname"].tolist(), p["flag"].tolist()) if fl != 4}
    assert have == want and len(have) > 100 and sorted(p["qname"].tolist()) == sorted(x[0] for x in asg)
    fasta = {l.split("\n")[0][1:].split()[0]: l.split("\n")[1] for l in (b[s + "consensus.fasta"].decode() for s in stems)}
    for x in np.nonzero(p["flag"] != 4)[0][::5]:
        nm, _ = walk_record(sam.cigar_ops(p["cigar"][x]), p["seq"][x], fasta[p["rname"][x]], int(p["pos"][x]))
        assert nm == p["nm"][x]
    # --write_sam needs --consensus
    with pytest.raises(SystemExit):
        _cli.cli(["--ont", "--fastq", sq, "--outfolder", str(tmp_path / "x"), "--write_sam"])


def test_cli_flag_under_fastq_dir_and_with_recruit(gpu_api, tmp_path):
    import shutil
    from ngspeciesid_amd import cli as _cli, fastpath
    d = tmp_path / "in"; d.mkdir()
    shutil.copy(os.path.join(GOLD, "sample_h1.fastq"), str(d / "h1.fastq"))
    synth.reads_to_fastq(synth.make_reads(synth.make_species(2, 600, 0.12, seed=81), 400, mu=15.0, seed=82, rc_fraction=0.3), str(d / "s_a.fastq"), prefix="a")
    res = []
    for flag in ([], ["--write_sam"]):
        out = str(tmp_path / ("o%d" % len(flag))); os.makedirs(out)
        args = _cli.build_parser().parse_args(["--ont", "--fastq_dir", str(d), "--outfolder", out, "--t", "1", "--consensus", "--racon", "--racon_iter", "1", "--recruit"] + flag); args.k, args.w = 13, 20
        fastpath.main(args, api=gpu_api)
        res.append(_files(out))
    a, b = res
    stems = sorted(f[:-len("consensus.fasta")] for f in a if f.endswith(os.sep + "consensus.fasta"))
    assert {s.split(os.sep)[0] for s in stems} == {"h1", "s_a"}
    assert sorted(set(b) - set(a)) == sorted(s + "reads_to_consensus.sam" for s in stems) and all(a[f] == b[f] for f in a if not f.endswith("logfile.txt"))
    for smp in ("h1", "s_a"):
        asg = [l.split("\t") for l in b[os.path.join(smp, "read_assignments.tsv")].decode().splitlines()][1:]
        for s in (x for x in stems if x.startswith(smp + os.sep)):
            p = _check_sam_file(os.path.join(str(tmp_path / "o1"), s + "reads_to_consensus.sam"), b[s + "consensus.fasta"], 20)
            cid = s.split("racon_cl_id_")[1].rstrip(os.sep)
            # every read recruited to this consensus is a record: the assigned ones mapped (but for the few the aligner finds no strand for), the ambiguous ones unmapped
            n_asg = sum(1 for x in asg if x[1] == cid and x[5] == "assigned"); n_amb = sum(1 for x in asg if x[1] == cid and x[5] == "ambiguous")
            assert len(p["qname"]) == n_asg + n_amb and 0.9 * n_asg <= (p["flag"] != 4).sum() <= n_asg
