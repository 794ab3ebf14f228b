"""CPU: the numpy restatement of ngsid_demux_scan (tests/demux_scan_reference.py) against the library's host locator, and the policy of `--demux_mid_tags`
(ngspeciesid_amd/demux.py): the patterns, interior hits, cuts, piece names, the refusals of the command line, and discard / split on a pool scanned by the reference
(demux_locate and demux_scan stubbed by the two references)."""
import ctypes as C
import logging, os, re
import numpy as np
import pytest
import demux_reference as ref
import demux_scan_reference as sref
from ngspeciesid_amd import demux
from ngspeciesid_amd._capi import Api, ReadSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def test_best_hit_of_the_reference_is_the_host_locator():
    """a few hundred random (read, pattern) pairs, IUPAC patterns and N in reads among them: where the pair has a hit, the one with the smallest (ed, end) has the
    locator's ed and end; where it has none, the locator reports none"""
    from ngspeciesid_amd import runtime
    fn = runtime.load_library().ngsid_host_infix_locate
    rng = np.random.default_rng(11)
    ed, st, en = C.c_int32(), C.c_int32(), C.c_int32()
    n_hit = n_multi = 0
    for case in range(300):
        iupac = case % 3 != 0
        m = int(rng.integers(1, 65)) if case % 5 else (1, 2, 63, 64)[case // 5 % 4]
        pat = _rand(rng, m, "ACGTRYNMKSWBDHVX" if case % 4 == 0 else "ACGT")
        read = _rand(rng, int(rng.integers(0, 400)), "ACGTN" if case % 2 else "ACGT")
        if case % 3 and len(read) > m:                                    # plant the pattern, sometimes twice, with a few substitutions
            for _ in range(1 + case % 2):
                p = int(rng.integers(0, len(read) - m + 1))
                conc = "".join(sref._SETS.get(c, c)[0] for c in pat)
                read = read[:p] + conc + read[p + m:]
        max_ed = int(rng.integers(0, 6)) if case % 7 else 70
        hit_off, hits = sref.scan([read], [pat], max_ed, iupac)
        assert fn(pat.encode(), C.c_int32(m), read.encode(), C.c_int32(len(read)), C.c_int32(max_ed), C.c_int32(int(iupac)), C.byref(ed), C.byref(st), C.byref(en)) == 0
        best = sref.best_hit(hit_off, hits, 0, 0)
        assert (best if best else (-1, -1)) == (ed.value, en.value), (case, pat, read, max_ed, iupac)
        n_hit += best is not None; n_multi += len(hits) > 1
        e = hits[:, 1]
        assert (np.diff(e) > 0).all() and (hits[:, 2] <= min(max_ed, m - 1)).all()
    assert n_hit > 100 and n_multi > 30


def test_runs_on_hand_made_rows():
    assert sref.runs_to_hits(np.array([0, 0, 0, 0]), 0) == [(0, 0)]                                  # A against AAAA: one run, the first position
    assert sref.runs_to_hits(sref.last_row("A", "ACAA"), 0) == [(0, 0), (2, 0)]
    assert sref.runs_to_hits(np.array([3, 2, 1, 1, 2, 9, 2, 0]), 2) == [(2, 1), (7, 0)]              # plateau: the first of the two 1s; a run open at the last base
    assert sref.runs_to_hits(np.array([1, 5, 1]), 1) == [(0, 1), (2, 1)]                             # one non-qualifying column between two runs
    assert sref.runs_to_hits(np.array([], dtype=np.int64), 3) == []
    off, hits = sref.scan(["", "ACGTACGT"], ["ACGT", "CGTA"], 0)
    assert off.tolist() == [0, 0, 3] and hits.tolist() == [[0, 3, 0], [1, 4, 0], [0, 7, 0]]          # ascending (end, pattern)


def test_scan_patterns_round_trip():
    sheet = demux.Sheet(["A", "B"], ["ACGTRYN", "MKSWBDHVX", "AAC"], [0, 2], [1, 1])
    pats = demux.scan_patterns(sheet)
    assert pats[:3] == sheet.tags and pats[3:] == ["NRYACGT", "XBDHVWSMK", "GTT"]
    assert [demux.revcomp_tag(p) for p in pats[3:]] == sheet.tags                                     # twice is the identity
    for a, b in zip("MRBDWSNX", "KYVHWSNX"):                                                          # the complement of a code is the code of the complements
        assert demux.revcomp_tag(a) == b and set(ref.revcomp(c) for c in sref._SETS[a]) == set(sref._SETS[b])
    assert ref.revcomp("ACGTTGCAAG") == demux.revcomp_tag("ACGTTGCAAG")


def test_interior_hits_on_hand_made_arrays():
    # one read of 200 bases, end tags cut at cut0 = 30 and cut1 = 25; patterns of 10 letters
    plen = [10, 10, 10, 10]
    hits = np.array([[0, 27, 1],      # the read's own forward tag: starts before cut0
                     [1, 39, 0],      # starts exactly at cut0: 39 - 10 - 0 + 1 = 30
                     [1, 40, 1],      # one edit: 40 - 10 - 1 + 1 = 30, still interior
                     [1, 39, 1],      # 39 - 10 - 1 + 1 = 29: not interior
                     [2, 174, 0],     # ends at L - cut1 - 1: interior
                     [3, 175, 0],     # ends at L - cut1: the read's own tail tag
                     [2, 100, 3]],    # beyond the bound
                    dtype=np.int32)
    got = demux.interior_hits([0, 7], hits, plen, [200], [30], [25], 2)
    assert got.tolist() == [False, True, True, False, True, False, False]
    assert demux.interior_hits([0, 7], hits, plen, [200], [30], [25], [2, 0, 3, 3]).tolist() == [False, True, False, False, True, False, True]      # a bound per pattern
    # a read without a located end tag has a cut of 0 on that side; the second read has no hit
    assert demux.interior_hits([0, 2, 2], hits[[0, 5]], plen, [200, 50], [0, 0], [0, 0], 2).tolist() == [True, True]
    assert demux.interior_hits([0, 0], np.zeros((0, 3), np.int32), plen, [10], [0], [0], 2).tolist() == []


@pytest.mark.parametrize("case", range(len(sref.CUT_CASES)))
def test_cuts_and_pieces(case):
    c = sref.CUT_CASES[case]
    cuts = demux.hit_cuts(np.array(c["hits"], dtype=np.int32), c["plen"], c["T"])
    assert cuts.tolist() == c["cuts"] and demux.pieces_of(cuts, c["L"]) == c["pieces"]


def test_piece_names():
    assert demux.piece_name("read7", 1) == "read7/p1"
    assert demux.piece_name("read7 s2 extra words", 3) == "read7/p3 s2 extra words"
    assert demux.piece_name("read7\tch=5", 12) == "read7/p12\tch=5"
    assert demux.piece_name("", 2) == "/p2"


def test_default_bound_by_tag_length():
    assert [demux.default_mid_max_ed(m) for m in (1, 8, 12, 13, 15, 16, 17, 23, 24, 40, 64)] == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 3]


# ---- the pool of the issue: four forward and four reverse tags of 24 bases, clean reads and two-amplicon concatemers, scanned by the reference
TAGS = ref.make_tags(8, 24, 9, seed=5)
FWD, REV = TAGS[0::2], TAGS[1::2]
NAMES = ["s_one", "s_two", "s_three", "s_four"]
N_CLEAN, N_CONC = 60, 30


@pytest.fixture(scope="module")
def pool():
    p = ref.make_pool(FWD, REV, 30, seed=3, junk_reads=0, max_edits=3)
    pairs = [(2 * i, 2 * i + 1) for i in range(N_CONC)]
    cs, cq = sref.make_concatemers(p, pairs)
    return dict(seqs=p["seqs"][:N_CLEAN] + cs, quals=p["quals"][:N_CLEAN] + cq, names=p["names"][:N_CLEAN] + ["conc%d x" % i for i in range(N_CONC)],
                sample=p["sample"], pairs=pairs)


@pytest.fixture(scope="module")
def sheet(tmp_path_factory):
    path = tmp_path_factory.mktemp("sheet") / "sheet.tsv"
    path.write_text("".join("%s\t%s\t%s\n" % x for x in zip(NAMES, FWD, REV)))
    return str(path)


@pytest.fixture(scope="module")
def pool_scan(pool, sheet):
    sh = demux.read_sheet(sheet)
    return sref.scan(pool["seqs"], demux.scan_patterns(sh), 3, True)


@pytest.fixture(scope="module")
def pool_locate(pool, sheet):
    return ref.locate(pool["seqs"], demux.read_sheet(sheet).tags, 150, 3, True)[0]


def test_clean_reads_have_two_end_hits_and_concatemers_two_interior_ones(pool, sheet, pool_scan, pool_locate):
    sh = demux.read_sheet(sheet)
    hit_off, hits = pool_scan
    lens = np.array([len(s) for s in pool["seqs"]])
    result = demux.assign(pool_locate, sh, 2, lens=lens)
    plen = [len(p) for p in demux.scan_patterns(sh)]
    inner = demux.interior_hits(hit_off, hits, plen, lens, result[3], result[4], demux.default_mid_max_ed(24))
    per_read = np.diff(hit_off.astype(np.int64))
    read = np.repeat(np.arange(len(lens)), per_read)
    n_inner = np.bincount(read[inner], minlength=len(lens))
    assert demux.default_mid_max_ed(24) == 3
    assert (per_read[:N_CLEAN] == 2).all() and (n_inner[:N_CLEAN] == 0).all()                       # exactly the two end tags, neither of them interior
    assert (per_read[N_CLEAN:] == 4).all() and (n_inner[N_CLEAN:] == 2).all()


def _stub(monkeypatch):
    def fake_locate(self, rs, tags, window=150, max_ed=3, iupac=True, matrices=False):
        reads = [rs.seq[int(rs.off[i]):int(rs.off[i + 1])].tobytes().decode() for i in range(rs.n)]
        h = ref.locate(reads, list(tags), window, max_ed, iupac)
        return h if matrices else h[0]

    def fake_scan(self, rs, patterns, max_ed=3, iupac=True, cap=None):
        reads = [rs.seq[int(rs.off[i]):int(rs.off[i + 1])].tobytes().decode() for i in range(rs.n)]
        return sref.scan(reads, list(patterns), max_ed, iupac)
    monkeypatch.setattr(Api, "demux_locate", fake_locate)
    monkeypatch.setattr(Api, "demux_scan", fake_scan)


def _args(extra):
    from ngspeciesid_amd import cli, pipeline
    a = cli.build_parser().parse_args(["--ont"] + extra); a.k, a.w = 13, 20
    if a.poa_single_below is None: a.poa_single_below = pipeline.SINGLE_BELOW
    return a


def _records(path):
    if not os.path.exists(path):
        return []
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % 4 == 0
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4)]


@pytest.fixture(scope="module")
def small(pool):
    """20 clean reads and 6 concatemers of the pool"""
    keep = list(range(20)) + list(range(N_CLEAN, N_CLEAN + 6))
    return dict(seqs=[pool["seqs"][i] for i in keep], quals=[pool["quals"][i] for i in keep], names=[pool["names"][i] for i in keep],
                truth=[tuple(int(pool["sample"][j]) for j in pool["pairs"][i]) for i in range(6)])


def _run(oracle, monkeypatch, tmp_path, small, sheet, extra, out):
    from ngspeciesid_amd import fastpath
    _stub(monkeypatch)
    fq = str(tmp_path / "pool.fastq"); ref.write_fastq(fq, small["names"], small["seqs"], small["quals"])
    res = fastpath.main(_args(["--fastq", fq, "--outfolder", str(tmp_path / out), "--t", "1", "--demux_sheet", sheet, "--demux_only"] + extra), api=oracle)
    files = {n: _records(str(tmp_path / out / "demux" / (n + ".fastq"))) for n in NAMES}
    summary = {l.split("\t")[1] if l.startswith("mid_tags=") else l.split("\t")[0]: l.split("\t")[-1] for l in open(str(tmp_path / out / "demux_summary.tsv")).read().splitlines() if not l.startswith("#")}
    return res, files, _records(str(tmp_path / out / "demux_unassigned.fastq")), summary


def test_off_discard_and_split_on_the_reference_scan(oracle, monkeypatch, tmp_path, small, sheet):
    res0, files0, un0, sum0 = _run(oracle, monkeypatch, tmp_path, small, sheet, [], "off")
    assert sorted(os.listdir(str(tmp_path / "off"))) == ["demux", "demux_summary.tsv", "demux_unassigned.fastq"] and not any(k.startswith("mid_tags") or "interior" in k for k in sum0)
    whole0 = sum(len(v) for v in files0.values())
    # discard: the six concatemers go whole to the unassigned file, status 5
    res1, files1, un1, sum1 = _run(oracle, monkeypatch, tmp_path, small, sheet, ["--demux_mid_tags", "discard"], "discard")
    conc = [(n, s, q) for n, s, q in zip(small["names"], small["seqs"], small["quals"]) if n.startswith("conc")]
    assert [r for r in un1 if r[0].startswith("conc")] == conc and not any(r[0].startswith("conc") for v in files1.values() for r in v)
    assert sum1["status=5"] == "6" and sum1["reads_with_interior_hits"] == "6" and sum1["pieces_made"] == "0"
    assert sum(len(v) for v in files1.values()) + len(un1) == len(small["seqs"])
    rows = [l.split("\t") for l in open(str(tmp_path / "discard" / "demux_concatemers.tsv")).read().splitlines() if not l.startswith("#")]
    assert [r[0] for r in rows] == ["conc%d" % i for i in range(6)] and all(int(r[1]) == len(s) for r, (_, s, _) in zip(rows, conc)) and all(len(r[3].split(",")) == 2 for r in rows)
    # split: every amplicon lands in its true sample's file, behind the whole reads; the original read is written nowhere
    res2, files2, un2, sum2 = _run(oracle, monkeypatch, tmp_path, small, sheet, ["--demux_mid_tags", "split", "--demux_mid_max_ed", "3"], "split")
    assert res2["demux"]["mid_tags"]["concatemers"] == 6
    everything = [r for v in files2.values() for r in v] + un2
    assert not any(r[0].split()[0] in ("conc%d" % i for i in range(6)) for r in everything)
    for i, (a, b) in enumerate(small["truth"]):
        where = {r[0].split()[0]: n for n, v in files2.items() for r in v if r[0].startswith("conc%d/" % i)}
        mine = sorted(where)
        assert where[mine[0]] == NAMES[a] and where[mine[-1]] == NAMES[b] and len(mine) == 2, (i, where)
        first = [r for r in files2[NAMES[a]] if r[0].split()[0] == mine[0]][0]
        assert first[0] == mine[0] + " x" and first[1] in small["seqs"][20 + i] and len(first[1]) == len(first[2]) and 250 < len(first[1]) < 420
    for n in NAMES:                                                                                   # whole reads first, in input order, then the pieces
        kinds = ["/p" in r[0].split()[0] for r in files2[n]]
        assert kinds == sorted(kinds) and [r for r in files2[n] if "/p" not in r[0].split()[0]] == files1[n]
    assert sum2["pieces_assigned"] == "12" and int(sum2["pieces_made"]) >= 12
    same = sum(a == b for a, b in small["truth"])
    assert sum2["concatemers_with_pieces_of_one_sample"] == str(same) and sum2["concatemers_with_pieces_of_several_samples"] == str(6 - same)
    rows = [l.split("\t") for l in open(str(tmp_path / "split" / "demux_concatemers.tsv")).read().splitlines() if not l.startswith("#")]
    for r, (a, b) in zip(rows, small["truth"]):
        got = [s for s in r[4].split(",") if s != "-"]
        assert got == [NAMES[a], NAMES[b]] and int(r[2]) == len(r[4].split(","))
    assert whole0 >= sum(len([r for r in v if "/p" not in r[0]]) for v in files2.values())


def test_cli_refusals(tmp_path, caplog, sheet):
    from ngspeciesid_amd import cli
    fq = str(tmp_path / "pool.fastq"); open(fq, "w").close()
    base = ["--ont", "--fastq", fq, "--outfolder", str(tmp_path / "o"), "--t", "1"]
    for argv, text in ((base + ["--demux_mid_tags", "split"], "need --demux_sheet"),
                       (base + ["--demux_mid_max_ed", "2"], "need --demux_sheet"),
                       (base + ["--demux_sheet", sheet, "--demux_mid_tags", "split", "--demux_mid_max_ed", "-1"], "--demux_mid_max_ed must not be negative"),
                       (base + ["--demux_sheet", sheet, "--demux_mid_max_ed", "2"], "--demux_mid_tags discard | split")):
        caplog.clear()
        with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as e:
            cli.cli(argv)
        assert e.value.code not in (0, None) and text in caplog.text, argv
    with pytest.raises(SystemExit) as e:                                                              # not one of off / discard / split
        cli.cli(base + ["--demux_sheet", sheet, "--demux_mid_tags", "maybe"])
    assert e.value.code not in (0, None)
    a = cli.build_parser().parse_args(["--ont", "--fastq", fq])
    assert a.demux_mid_tags == "off" and a.demux_mid_max_ed is None
    assert not os.path.exists(str(tmp_path / "o" / "demux"))


def test_a_library_without_the_kernel_is_an_error(oracle):
    from ngspeciesid_amd._capi import NgsidError
    with pytest.raises(NgsidError):
        oracle.demux_scan(ReadSet.from_strings(["ACGT"]), ["AC"])


def test_header_declares_and_library_exports_the_call():
    text = open(os.path.join(ROOT, "include", "ngsid_demux.h")).read()
    assert re.search(r"int32_t\s+ngsid_demux_scan\s*\(", text) and "ngsid_demux_scan_params_t" in text
    from ngspeciesid_amd import runtime
    lib = runtime.load_library()
    assert hasattr(lib, "ngsid_demux_scan") and lib.ngsid_abi_version() == 2
