"""GPU: ngsid_demux_scan (include/ngsid_demux.h, csrc/k_demux_scan.hip) through Api.demux_scan against tests/demux_scan_reference.py, array for array, on the smallest
shapes at which the kernel can go wrong; the last test runs `--demux_mid_tags` of the command line on a pool with six hand-made concatemers."""
import os
import numpy as np
import pytest
import demux_reference as ref
import demux_scan_reference as sref
from ngspeciesid_amd import runtime
from ngspeciesid_amd._capi import ReadSet, NgsidError

pytestmark = pytest.mark.gpu
CHUNK = 128          # DSC_CHUNK of k_demux_scan.hip: letters of a read staged at a time


def _rand(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def _same(got, want, what):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.int32 and got[1].shape[1:] == (3,)
    assert np.array_equal(got[0], want[0]), "%s: hit_off differs at read %s" % (what, np.flatnonzero(got[0] != want[0])[:3].tolist())
    bad = np.argwhere(got[1] != want[1])
    assert len(bad) == 0, "%s: hit %d differs: got %s, want %s" % (what, bad[0][0], got[1][bad[0][0]].tolist(), want[1][bad[0][0]].tolist())


def _check(api, reads, patterns, max_ed, iupac=True, what=""):
    want = sref.scan(reads, patterns, max_ed, iupac)
    got = api.demux_scan(ReadSet.from_strings(reads), patterns, max_ed=max_ed, iupac=iupac)
    _same(got, want, "%s max_ed=%d iupac=%d" % (what, max_ed, iupac))
    return want


def test_source_states_the_staging_chunk():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ngspeciesid_amd", "csrc", "k_demux_scan.hip")).read()
    assert "#define DSC_CHUNK %d " % CHUNK in text


@pytest.mark.parametrize("P", [1, 2, 3, 64, 65, 130])
def test_pattern_counts(gpu_api, P):
    """several reads of unequal lengths per wave below 64 patterns (a length-0 read between long ones), the pass boundary, a nearly empty last pass; more than one
    workgroup throughout"""
    rng = np.random.default_rng(500 + P)
    patterns = [_rand(rng, int(rng.integers(5, 15))) for _ in range(P)]
    n = 300 if P <= 3 else 14
    reads = []
    for i in range(n):
        r = _rand(rng, int(rng.integers(1, 330)) if i % 3 else int(rng.integers(200, 330)))
        for _ in range(i % 4):                                           # up to three planted patterns, the last pattern among them
            t = patterns[P - 1 if i % 8 == 3 else int(rng.integers(0, P))]
            p = int(rng.integers(0, len(r) + 1)); r = r[:p] + t + r[p:]
        reads.append(r)
    reads[1] = ""; reads[5] = ""; reads[n - 1] = ""                      # between long reads, and as the last read
    want = _check(gpu_api, reads, patterns, 1, what="P=%d" % P)
    assert len(want[1]) > n and (want[1][:, 0] == P - 1).any() and (np.diff(want[0].astype(np.int64)) > 2).any()


def test_pattern_lengths_read_lengths_and_the_clamp(gpu_api):
    """patterns of 1, 63 and 64 letters (the top bit); reads of 0 .. 9 letters and around the first two multiples of the staging chunk, the pattern planted across
    the chunk boundary and at both ends; max_ed 0, 3 and above every pattern length (clamped to m - 1: every position of a read qualifies, one run per read)"""
    rng = np.random.default_rng(600)
    base = _rand(rng, 64)
    patterns = ["A", base[:63], base, base[:9]]
    lens = list(range(10)) + [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1]
    reads = [_rand(rng, L) for L in lens]
    put = lambda r, p, t: r[:p] + t + r[p + len(t):] if 0 <= p and p + len(t) <= len(r) else r
    for L in lens[10:]:
        r = _rand(rng, L)
        reads.append(put(r, 0, base))                                    # at the head
        reads.append(put(r, L - 64, base))                               # the last column of the read
        reads.append(put(r, CHUNK - 30, base[:63]))                      # across the first chunk boundary (the longer reads)
        reads.append(put(r, 2 * CHUNK - 5, base[:9]))                    # across the second
        reads.append(put(r, CHUNK - 9, base[:9]))                        # ends in the last column of the first chunk
        reads.append(put(r, CHUNK, base[:9]))                            # starts in the first column of the second
    assert all(len(r) in lens for r in reads)
    for max_ed in (0, 3, 70):
        want = _check(gpu_api, reads, patterns, max_ed, what="lengths")
    off, hits = want                                                     # max_ed 70: k = m - 1 for every pattern
    r = len(lens) + 1                                                    # a read of CHUNK - 1 letters that ends with the 64-letter pattern
    mine = hits[int(off[r]):int(off[r + 1])]
    assert mine[mine[:, 0] == 2].tolist() == [[2, CHUNK - 2, 0]]


def test_run_shapes(gpu_api):
    """hand-made rows: a run open at column 0, one open at the last base, two runs separated by one non-qualifying column, a plateau tie (the first position),
    `A` against AAAA and ACAA at max_ed 0"""
    got = gpu_api.demux_scan(ReadSet.from_strings(["AAAA", "ACAA", "", "C"]), ["A"], max_ed=0)
    assert got[0].tolist() == [0, 1, 3, 3, 3] and got[1].tolist() == [[0, 0, 0], [0, 0, 0], [0, 2, 0]]
    pat = "ACGTTGCA"
    reads = [pat + "TTTTTTTTTT",                   # a run open at column 0 ... (with max_ed 2 the first qualifying column is a prefix of the pattern)
             "TTTTTTTTTT" + pat,                   # ... and one open at the last base
             "TTTTTTTTTT" + pat[:-1],              # the read ends inside the pattern: the run is closed at L
             "GG" + pat + "CCCCCCCCCC" + pat,      # two occurrences
             "TTTT" + "ACGTTGC" + "TTTT",          # plateau: the last letter missing
             pat[1:] + "CCCC" + pat[:-1]]
    for max_ed in (0, 1, 2, 7, 8):
        want = _check(gpu_api, reads, [pat, "AC", "CA"], max_ed, what="runs")
    want = sref.scan(["ACAC"], ["AC"], 0)
    assert want[1].tolist() == [[0, 1, 0], [0, 3, 0]]                    # columns 1 and 3 qualify, column 2 does not: two runs
    _check(gpu_api, ["ACAC", "ACACAC", "CACA"], ["AC"], 0, what="one column between two runs")
    s = sref.last_row("ACGT", "TTACGGTT")
    assert s.tolist().count(1) >= 2 and sref.runs_to_hits(s, 1)[0][0] == int(np.argmax(s == 1))      # a tie within the run: the first position
    _check(gpu_api, ["TTACGGTT", "ACGGT", "TTACG"], ["ACGT"], 1, what="plateau")


CODES = {"R": "AG", "Y": "CT", "N": "ACGT", "X": "ACGT", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "M": "AC", "K": "GT", "S": "CG", "W": "AT"}


def test_iupac_and_n_in_reads(gpu_api):
    rng = np.random.default_rng(700)
    patterns = ["ACGTRYACGTAC", "NNACGTTGCANN", "ACBDHVACGTTT", "GGMKSWGGATCC", "XACGTTTGGA"]
    reads = []
    for i in range(60):
        r = _rand(rng, int(rng.integers(40, 300)), "ACGTN" if i % 3 == 0 else "ACGT")
        if i % 2 == 0:
            t = patterns[i % len(patterns)]
            conc = "".join(CODES.get(c, c)[int(rng.integers(0, len(CODES.get(c, c))))] for c in t)
            r = r[:17] + conc + r[17:]
            if i % 4 == 0: r = r[:19] + "N" + r[20:]
        reads.append(r)
    on = _check(gpu_api, reads, patterns, 2, iupac=True, what="iupac")
    off = _check(gpu_api, reads, patterns, 2, iupac=False, what="no iupac")
    assert len(on[1]) > len(off[1]) and (np.diff(on[0].astype(np.int64))[0::2] >= 1).all()


def test_residency_capacity_and_chunking():
    rng = np.random.default_rng(800)
    tags = [_rand(rng, 20) for _ in range(12)]
    patterns = tags + [ref.revcomp(t) for t in tags]
    reads = []
    for i in range(700):
        a = _rand(rng, int(rng.integers(0, 420)))
        if i % 5: a = tags[int(rng.integers(0, 12))] + a + ref.revcomp(tags[int(rng.integers(0, 12))])
        if i % 50 == 7: a = a + a
        reads.append(a)
    rs = ReadSet.from_strings(reads)
    with runtime.new_api() as api:
        plain = api.demux_scan(rs, patterns, max_ed=2)
        H = len(plain[1])
        assert H > 1000
        assert len(api.demux_scan(rs, patterns, max_ed=2, cap=H)[1]) == H and len(api.demux_scan(rs, patterns, max_ed=2, cap=H + 100)[1]) == H     # one call with room
        for cap in (H - 1, 1, 0):
            with pytest.raises(NgsidError) as e:
                api.demux_scan(rs, patterns, max_ed=2, cap=cap)
            assert e.value.code == -4 and e.value.needed == H
        dev = api.upload_reads(rs)
        try:
            on_dev = api.demux_scan(dev, patterns, max_ed=2)
            api.set_option("demux_scan_chunk_reads", 97)                 # 8 chunks, the last one short
            chunked = api.demux_scan(rs, patterns, max_ed=2)
            api.set_option("demux_scan_chunk_reads", 1)
            by_one = api.demux_scan(dev, patterns, max_ed=2)
            api.set_option("demux_scan_chunk_reads", 0)
        finally:
            dev.release()
    for other, what in ((on_dev, "device-resident"), (chunked, "chunks of 97"), (by_one, "chunks of 1")):
        assert other[0].tobytes() == plain[0].tobytes() and other[1].tobytes() == plain[1].tobytes(), what
    sub = list(range(0, 700, 23))
    want = sref.scan([reads[i] for i in sub], patterns, 2)
    got = [plain[1][int(plain[0][i]):int(plain[0][i + 1])] for i in sub]
    assert np.array_equal(np.concatenate(got), want[1]) and [len(g) for g in got] == np.diff(want[0].astype(np.int64)).tolist()


def test_argument_errors_and_empty_sets(gpu_api):
    rs = ReadSet.from_strings(["ACGTACGTAC", "ACGTaCGTAC"])
    for kw, code in ((dict(patterns=["ACGT"]), -3), (dict(patterns=["A" * 65]), -6), (dict(patterns=[]), -2), (dict(patterns=["ACGT"], max_ed=-1), -2),
                     (dict(patterns=["ACGTAC"] * 8193), -2)):
        with pytest.raises(NgsidError) as e:
            gpu_api.demux_scan(rs, **kw)
        assert e.value.code == code, kw
    empty_pattern = ReadSet(np.frombuffer(b"ACGT", dtype=np.uint8), None, np.array([0, 4, 4], dtype=np.uint64))
    with pytest.raises(NgsidError) as e:
        gpu_api.demux_scan(rs, empty_pattern)
    assert e.value.code == -2
    off, hits = gpu_api.demux_scan(ReadSet.from_strings([]), ["ACGT"])                             # an empty read set is legal
    assert off.tolist() == [0] and hits.shape == (0, 3)
    off, hits = gpu_api.demux_scan(ReadSet.from_strings(["", ""]), ["ACGT"])
    assert off.tolist() == [0, 0, 0] and hits.shape == (0, 3)
    off, hits = gpu_api.demux_scan(ReadSet.from_strings(["ACGTACGTAC"]), ["G" * 64, "ACGTAC"] * 4096, max_ed=0)      # the largest pattern list
    odd = np.arange(1, 8192, 2)                                                                     # ACGTAC ends at 5 and at 9: ascending (end, pattern)
    assert off.tolist() == [0, 8192] and hits[:, 0].tolist() == np.concatenate((odd, odd)).tolist() and hits[:, 1].tolist() == [5] * 4096 + [9] * 4096 and not hits[:, 2].any()


# ---- the command line
def _records(path):
    if not os.path.exists(path):
        return []
    lines = open(path).read().split("\n")
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4)]


def test_cli_mid_tags_split_discard_and_off(gpu_api, tmp_path):
    """4 dual-tag samples over 2 forward x 2 reverse tags (every pair of tags is a sample, so the outer tags of a concatemer of two samples form a sheet pair),
    12 reads each, and six concatemers"""
    from ngspeciesid_amd.cli import cli
    tags = ref.make_tags(4, 24, 9, seed=5)
    fwd, rev = [tags[0], tags[1], tags[0], tags[1]], [tags[2], tags[3], tags[3], tags[2]]
    names = ["s_one", "s_two", "s_mixA", "s_mixB"]
    pool = ref.make_pool(fwd, rev, 14, seed=21, n_species=2, length=320, junk_reads=0, mu=20.0, rc_fraction=0.3, max_edits=2)
    plus = {s: np.flatnonzero((pool["sample"] == s) & (pool["strand"] == 0)).tolist() for s in range(4)}
    assert all(len(v) >= 4 for v in plus.values())
    rc = lambda sq: (ref.revcomp(sq[0]), sq[1][::-1])
    one = lambda i: (pool["seqs"][i], pool["quals"][i])
    join = lambda parts: ("".join(p[0] for p in parts), "".join(p[1] for p in parts))
    made = [(join([one(plus[0][0]), one(plus[1][0])]), [0, 1]),                          # two samples joined: its outer tags are those of s_mixA
            (join([one(plus[1][1]), one(plus[1][2])]), [1, 1]),                          # one sample twice
            (join([one(plus[2][0]), one(plus[3][0]), one(plus[0][1])]), [2, 3, 0]),      # three pieces
            (rc(join([one(plus[3][1]), one(plus[2][1])])), [2, 3]),                      # reverse-complemented as a whole: the pieces come in reverse order
            (join([one(plus[1][3]), one(plus[0][2])]), [1, 0]),                          # outer tags of s_mixB
            (join([rc(one(plus[2][2])), rc(one(plus[3][2]))]), [2, 3])]                  # each amplicon on the reverse strand
    truth = [t for _, t in made]
    used = {plus[0][0], plus[1][0], plus[1][1], plus[1][2], plus[2][0], plus[3][0], plus[0][1], plus[3][1], plus[2][1], plus[1][3], plus[0][2], plus[2][2], plus[3][2]}
    clean = [i for i in range(len(pool["seqs"])) if i not in used]
    all_names = [pool["names"][i] for i in clean] + ["conc%d len=%d" % (c, len(sq[0])) for c, (sq, _) in enumerate(made)]
    all_seqs = [pool["seqs"][i] for i in clean] + [sq[0] for sq, _ in made]; all_quals = [pool["quals"][i] for i in clean] + [sq[1] for sq, _ in made]
    n_conc = 6
    fq = str(tmp_path / "pool.fastq"); ref.write_fastq(fq, all_names, all_seqs, all_quals)
    sheet_path = str(tmp_path / "sheet.tsv")
    open(sheet_path, "w").write("".join("%s\t%s\t%s\n" % x for x in zip(names, fwd, rev)))
    base = ["--ont", "--fastq", fq, "--demux_sheet", sheet_path, "--t", "1", "--demux_only"]

    def run(out, extra):
        cli(base + ["--outfolder", str(tmp_path / out)] + extra)
        files = {n: _records(str(tmp_path / out / "demux" / (n + ".fastq"))) for n in names}
        summary = {l.split("\t")[1] if l.startswith("mid_tags=") else l.split("\t")[0]: l.split("\t")[-1]
                   for l in open(str(tmp_path / out / "demux_summary.tsv")).read().splitlines() if not l.startswith("#")}
        return files, _records(str(tmp_path / out / "demux_unassigned.fastq")), summary

    # ---- without the flag: the concatemer of s_one and s_two has the outer tags of s_mixA and sits whole in that sample's file
    files, un, summary = run("off", [])
    assert not os.path.exists(str(tmp_path / "off" / "demux_concatemers.tsv")) and not any("interior" in k or k.startswith("pieces") for k in summary)
    wrong = [r for r in files["s_mixA"] if r[0].startswith("conc0 ")]
    assert len(wrong) == 1 and len(wrong[0][1]) > 600 and wrong[0][1] in all_seqs[all_names.index(wrong[0][0])]
    # ---- split
    files, un, summary = run("split", ["--demux_mid_tags", "split"])
    written = [r for v in files.values() for r in v] + un
    assert not any(r[0].split()[0] == "conc%d" % c for r in written for c in range(n_conc))          # the original read is written nowhere
    rows = [l.split("\t") for l in open(str(tmp_path / "split" / "demux_concatemers.tsv")).read().splitlines() if not l.startswith("#")]
    assert [r[0] for r in rows] == ["conc%d" % c for c in range(n_conc)]                              # the six, and no clean read
    for c, r in enumerate(rows):
        whole = all_seqs[all_names.index([nm for nm in all_names if nm.split()[0] == "conc%d" % c][0])]
        assert int(r[1]) == len(whole) and int(r[2]) == len(r[4].split(",")) and len(r[3].split(",")) >= 2 * (len(truth[c]) - 1)
        assert [s for s in r[4].split(",") if s != "-"] == [names[s] for s in truth[c]], (c, r)
        where = [(rec[0].split()[0], n, rec) for n, v in files.items() for rec in v if rec[0].startswith("conc%d/p" % c)]
        assert [n for _, n, _ in sorted(where)] == [names[s] for s in truth[c]]                       # every amplicon in its true sample's file
        for _, _, rec in where:
            assert rec[1] in whole and len(rec[1]) == len(rec[2]) and 250 < len(rec[1]) < 420 and all(t not in rec[1] for t in tags)
    n_pieces = sum(len(t) for t in truth)
    assert summary["reads_with_interior_hits"] == str(n_conc) and summary["pieces_assigned"] == str(n_pieces) and int(summary["pieces_made"]) >= n_pieces
    one = sum(len(set(t)) == 1 for t in truth)
    assert summary["concatemers_with_pieces_of_one_sample"] == str(one) and summary["concatemers_with_pieces_of_several_samples"] == str(n_conc - one)
    assert summary["status=5"] == str(n_conc)
    for n in names:                                                                                   # pieces behind the whole reads
        kinds = ["/p" in r[0].split()[0] for r in files[n]]
        assert kinds == sorted(kinds)
    # ---- discard
    files, un, summary = run("discard", ["--demux_mid_tags", "discard"])
    conc = [(nm, s, q) for nm, s, q in zip(all_names, all_seqs, all_quals) if nm.startswith("conc")]
    assert [r for r in un if r[0].startswith("conc")] == conc and not any(r[0].startswith("conc") for v in files.values() for r in v)
    assert summary["status=5"] == str(n_conc) and "mid_tag" in open(str(tmp_path / "discard" / "demux_summary.tsv")).read()
    assert len(open(str(tmp_path / "discard" / "demux_concatemers.tsv")).read().splitlines()) == n_conc + 1
