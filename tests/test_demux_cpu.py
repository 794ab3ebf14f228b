"""CPU: the policy layer of the demultiplexer (ngspeciesid_amd/demux.py) - the sheet reader, assign() on hand-written hits, the generator's truth recovered through the
oracle's locator, the writers and the summary with a stubbed demux_locate (the stub is tests/demux_reference.py), and the refusals of the command line."""
import logging, os, re
import numpy as np
import pytest
import demux_reference as ref
from ngspeciesid_amd import demux
from ngspeciesid_amd._capi import Api, ReadSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0, T1, T2, T3 = "ACGTACGTAAGG", "TTGGCCAATTCC", "GATTACAGATTA", "CCCCAAAATTTG"


def _sheet(tmp_path, text, name="sheet.tsv"):
    p = tmp_path / name; p.write_text(text)
    return str(p)


def test_read_sheet_good_forms(tmp_path):
    s = demux.read_sheet(_sheet(tmp_path, "# kit\n\nA\t%s\t%s\nB\t%s\t%s\r\nC\t%s\t%s\n" % (T0, T1, T0, T2, T3, T1)))
    assert s.dual and s.samples == ["A", "B", "C"] and s.tags == [T0, T1, T2, T3]           # identical strings share one index
    assert s.fwd.tolist() == [0, 0, 3] and s.rev.tolist() == [1, 2, 1]
    for text in ("A\t%s\nB\t%s\n" % (T0, T1), "A\t%s\t\nB\t%s\t\n" % (T0, T1), "A\t%s\nB\t%s\t\n" % (T0, T1)):      # third column absent or empty
        s = demux.read_sheet(_sheet(tmp_path, text))
        assert not s.dual and s.rev is None and s.fwd.tolist() == [0, 1]
    s = demux.read_sheet(_sheet(tmp_path, "A\tACGTRYN\tMKSWBDHVX\n"))
    assert s.tags == ["ACGTRYN", "MKSWBDHVX"]
    assert demux.read_sheet(_sheet(tmp_path, "A\t%s\t%s\n" % ("A" * 64, T1))).tags[0] == "A" * 64


@pytest.mark.parametrize("text,row,what", [
    ("A\t%s\t%s\nA\t%s\t%s\n" % (T0, T1, T2, T3), 2, "twice"),                                # duplicate sample name
    ("A\t%s\t%s\nsub/B\t%s\t%s\n" % (T0, T1, T2, T3), 2, "plain file name"),
    ("..\t%s\t%s\n" % (T0, T1), 1, "plain file name"),
    ("A\t%s\t%s\n#c\nB\t%s\t%s\n" % (T0, T1, T0, T1), 3, "has the tags of"),                  # the same ordered pair
    ("A\t%s\t%s\nB\t%s\t%s\n" % (T0, T1, T1, T0), 2, "other way round"),                      # (a, b) next to (b, a)
    ("A\t%s\nB\t%s\n" % (T0, T0), 2, "has the tags of"),                                      # single-ended: the same tag
    ("A\t%s\t%s\nB\t%s\n" % (T0, T1, T2), 2, "some rows"),                                    # mixture
    ("A\t%s\nB\t%s\t%s\n" % (T0, T2, T1), 2, "some rows"),
    ("A\tACGU\t%s\n" % T1, 1, "alphabet"), ("A\tacgt\t%s\n" % T1, 1, "alphabet"), ("A\t%s\tAC-T\n" % T0, 1, "alphabet"),
    ("A\t%s\t%s\n" % ("A" * 65, T1), 1, "longer than 64"),
    ("A\n", 1, "expected"),
])
def test_read_sheet_rejects(tmp_path, text, row, what):
    with pytest.raises(ValueError) as e:
        demux.read_sheet(_sheet(tmp_path, text))
    assert "row %d" % row in str(e.value) and what in str(e.value)


def _hit(tag=-1, ed=-1, start=-1, end=-1, ed2=-1):
    return [tag, ed, start, end, ed2]


DUAL = demux.Sheet(["A", "B"], [T0, T1, T2, T3], [0, 2], [1, 3])
SINGLE = demux.Sheet(["A", "B"], [T0, T1], [0, 1], None)


def test_assign_dual_statuses_strands_margin_and_cuts():
    hits = np.array([
        [_hit(0, 1, 5, 16, -1), _hit(1, 0, 2, 13, -1)],        # 0: A, strand 0
        [_hit(1, 0, 0, 11, -1), _hit(0, 2, 3, 14, -1)],        # 1: A, strand 1
        [_hit(2, 0, 0, 11, 2), _hit(3, 1, 0, 11, 3)],          # 2: B, margins exactly min_margin
        [_hit(2, 0, 0, 11, 1), _hit(3, 1, 0, 11, 3)],          # 3: one below the margin on side 0 -> ambiguous
        [_hit(2, 1, 0, 11, 1), _hit(3, 1, 0, 11, -1)],         # 4: tie (ed2 == ed) -> ambiguous
        [_hit(), _hit(1, 0, 2, 13, -1)],                       # 5: side 0 has no tag
        [_hit(0, 0, 0, 11, -1), _hit()],                       # 6: side 1 has no tag
        [_hit(), _hit(1, 3, 0, 11, 3)],                        # 7: no tag beats ambiguous
        [_hit(0, 0, 0, 11, -1), _hit(3, 0, 0, 11, -1)],        # 8: (A fwd, B rev): not in the sheet
        [_hit(0, 0, 0, 11, -1), _hit(0, 0, 0, 11, -1)],        # 9: (a, a): not in the sheet
        [_hit(0, 0, 0, 11, -1), _hit(1, 0, 0, 11, -1)],        # 10: A, but the read is 24 bases: nothing left
        [_hit(0, 0, 0, 11, -1), _hit(1, 0, 0, 11, -1)],        # 11: A, 25 bases: one base left
    ], dtype=np.int32)
    lens = np.array([400, 400, 400, 400, 400, 400, 400, 400, 400, 400, 24, 25])
    sample, strand, status, c0, c1 = demux.assign(hits, DUAL, 2, lens=lens)
    assert status.tolist() == [0, 0, 0, 2, 2, 1, 1, 1, 3, 3, 4, 0]
    assert sample.tolist() == [0, 0, 1, -1, -1, -1, -1, -1, -1, -1, -1, 0]
    assert strand.tolist() == [0, 1, 0, -1, -1, -1, -1, -1, -1, -1, -1, 0]
    assert c0.tolist() == [17, 12, 12, 12, 12, 0, 12, 0, 12, 12, 12, 12] and c1.tolist() == [14, 15, 12, 12, 12, 14, 0, 12, 12, 12, 12, 12]
    # a wider margin turns read 2 ambiguous, margin 0 accepts the tie; without lens nothing is status 4
    assert demux.assign(hits, DUAL, 3, lens=lens)[2].tolist()[2] == 2
    assert demux.assign(hits, DUAL, 0, lens=lens)[2].tolist()[3:5] == [0, 0]
    assert demux.assign(hits, DUAL, 2)[2].tolist()[10] == 0


def test_assign_single_ended():
    hits = np.array([
        [_hit(0, 1, 0, 11, -1), _hit()],                       # A, strand 0
        [_hit(), _hit(1, 0, 4, 15, 2)],                        # B, strand 1, margin exactly 2
        [_hit(), _hit()],                                      # no tag
        [_hit(0, 2, 0, 11, 3), _hit()],                        # one below the margin
        [_hit(0, 0, 0, 11, -1), _hit(1, 0, 0, 11, -1)],        # a tag on both ends
        [_hit(1, 0, 0, 11, -1), _hit()],                       # 12 bases: nothing left
    ], dtype=np.int32)
    sample, strand, status, c0, c1 = demux.assign(hits, SINGLE, 2, lens=np.array([300, 300, 300, 300, 300, 12]))
    assert status.tolist() == [0, 0, 1, 2, 3, 4] and sample.tolist() == [0, 1, -1, -1, -1, -1] and strand.tolist() == [0, 1, -1, -1, -1, -1]
    assert c0.tolist() == [12, 0, 0, 12, 12, 12] and c1.tolist() == [0, 16, 0, 0, 12, 0]


# ---- the generator's truth through the oracle's locator
TAGS = ref.make_tags(8, 24, 9, seed=5)
FWD, REV = TAGS[0::2], TAGS[1::2]
NAMES = ["s_one", "s_two", "s_three", "s_empty"]


def _sheet_text():
    return "".join("%s\t%s\t%s\n" % (n, f, r) for n, f, r in zip(NAMES, FWD, REV))


def test_tag_set_is_far_apart():
    for i, t in enumerate(TAGS):
        for j, u in enumerate(TAGS):
            if i != j: assert ref.edit_distance(t, u) >= 9
            assert ref.edit_distance(t, ref.revcomp(u)) >= 9


@pytest.fixture(scope="module")
def pool():
    return ref.make_pool(FWD, REV, 40, seed=7, junk_reads=6, samples=[0, 1, 2])


@pytest.fixture(scope="module")
def pool_hits(oracle, pool):
    return ref.locate(pool["seqs"], TAGS, 150, 3, True, lib=oracle.lib, prefix="ongsid_")


def test_truth_is_recovered_with_the_oracle_locator(tmp_path, pool, pool_hits):
    sheet = demux.read_sheet(_sheet(tmp_path, _sheet_text()))
    assert sheet.tags == TAGS
    sample, strand, status, c0, c1 = demux.assign(pool_hits[0], sheet, 2, lens=np.array([len(s) for s in pool["seqs"]]))
    good = ~pool["junk"] & (pool["edits"].max(axis=1) <= 3)
    assert good.sum() > 60 and (pool["strand"][good] == 1).any() and (pool["strand"][good] == 0).any()
    assert (status[good] == 0).all() and np.array_equal(sample[good], pool["sample"][good]) and np.array_equal(strand[good], pool["strand"][good])
    assert pool["junk"].sum() == 18 and (status[pool["junk"]] == 1).all()
    # the cut lies behind the tag: the kept part of a good read is inside its amplicon
    assert (c0[good] >= 20).all() and (c0[good] <= 30 + 24 + 4).all() and (c1[good] >= 20).all()


def test_host_locator_equals_oracle_locator(pool, pool_hits):
    sub = pool["seqs"][:25]
    got = ref.locate(sub, TAGS, 150, 3, True)
    for a, b in zip(got, pool_hits):
        assert np.array_equal(a, b[:25])


# ---- writers and summary, demux_locate stubbed by the reference
def _stub(monkeypatch, oracle):
    def fake(self, rs, tags, window=150, max_ed=3, iupac=True, matrices=False):
        reads = [rs.seq[int(rs.off[i]):int(rs.off[i + 1])].tobytes().decode() for i in range(rs.n)]
        h = ref.locate(reads, list(tags), window, max_ed, iupac, lib=oracle.lib, prefix="ongsid_")
        return h if matrices else h[0]
    monkeypatch.setattr(Api, "demux_locate", fake)


def _args(extra):
    from ngspeciesid_amd import cli, pipeline
    a = cli.build_parser().parse_args(["--ont"] + extra); a.k, a.w = 13, 20
    if a.poa_single_below is None: a.poa_single_below = pipeline.SINGLE_BELOW
    return a


def _records(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % 4 == 0
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4)]


@pytest.mark.parametrize("keep_tags", [False, True])
def test_demux_only_writes_samples_unassigned_and_summary(oracle, monkeypatch, tmp_path, pool, pool_hits, keep_tags):
    from ngspeciesid_amd import fastpath
    _stub(monkeypatch, oracle)
    fq = str(tmp_path / "pool.fastq"); ref.write_fastq(fq, pool["names"], pool["seqs"], pool["quals"])
    out = tmp_path / "out"
    res = fastpath.main(_args(["--fastq", fq, "--outfolder", str(out), "--t", "1", "--demux_sheet", _sheet(tmp_path, _sheet_text()), "--demux_only"] + (["--demux_keep_tags"] if keep_tags else [])), api=oracle)
    assert res["demux"]["reads"] == len(pool["seqs"])
    assert sorted(os.listdir(str(out))) == ["demux", "demux_summary.tsv", "demux_unassigned.fastq"]          # --demux_only: the three outputs and nothing else
    assert sorted(os.listdir(str(out / "demux"))) == ["s_one.fastq", "s_three.fastq", "s_two.fastq"]          # the empty sample gets no file
    sheet = demux.read_sheet(_sheet(tmp_path, _sheet_text()))
    sample, strand, status, c0, c1 = demux.assign(pool_hits[0], sheet, 2, lens=np.array([len(s) for s in pool["seqs"]]))
    seen = 0
    for s, name in enumerate(NAMES[:3]):
        want = [(pool["names"][i], pool["seqs"][i] if keep_tags else pool["seqs"][i][c0[i]:len(pool["seqs"][i]) - c1[i]],
                 pool["quals"][i] if keep_tags else pool["quals"][i][c0[i]:len(pool["seqs"][i]) - c1[i]]) for i in np.flatnonzero(sample == s)]
        assert _records(str(out / "demux" / (name + ".fastq"))) == want and len(want) >= 20          # input order, headers unchanged
        seen += len(want)
    un = _records(str(out / "demux_unassigned.fastq"))
    assert un == [(pool["names"][i], pool["seqs"][i], pool["quals"][i]) for i in np.flatnonzero(sample < 0)] and seen + len(un) == len(pool["seqs"])
    rows = [l.split("\t") for l in open(str(out / "demux_summary.tsv")).read().splitlines() if not l.startswith("#")]
    by = {r[0]: r[1:] for r in rows}
    tag_ed = np.where(pool_hits[0][:, :, 0] >= 0, pool_hits[0][:, :, 1], 0).sum(axis=1)
    for s, name in enumerate(NAMES):
        m = sample == s
        assert by[name] == [str(int(m.sum())), str(int((m & (strand == 0)).sum())), str(int((m & (strand == 1)).sum())), str(int(tag_ed[m].sum()))]
    assert by["s_empty"] == ["0", "0", "0", "0"]
    for st in (1, 2, 3, 4):
        c = int((status == st).sum())
        assert (("status=%d" % st) in by) == (c > 0)
        if c: assert by["status=%d" % st][-1] == str(c)
    assert int(by["status=1"][-1]) >= 18


def test_handover_to_the_fastq_dir_path(oracle, monkeypatch, tmp_path, pool):
    """without --demux_only the sample files run through _main_samples: <outfolder>/<sample>/ holds what --fastq_dir on <outfolder>/demux writes"""
    from ngspeciesid_amd import fastpath
    _stub(monkeypatch, oracle)
    fq = str(tmp_path / "pool.fastq"); ref.write_fastq(fq, pool["names"], pool["seqs"], pool["quals"])
    sheet = _sheet(tmp_path, _sheet_text())
    fastpath.main(_args(["--fastq", fq, "--outfolder", str(tmp_path / "a"), "--t", "1", "--demux_sheet", sheet]), api=oracle)
    fastpath.main(_args(["--fastq_dir", str(tmp_path / "a" / "demux"), "--outfolder", str(tmp_path / "b"), "--t", "1"]), api=oracle)
    for name in NAMES[:3]:
        fa, fb = sorted(os.listdir(str(tmp_path / "a" / name))), sorted(os.listdir(str(tmp_path / "b" / name)))
        assert fa == fb and "final_clusters.tsv" in fa
        for f in fa:
            assert open(str(tmp_path / "a" / name / f), "rb").read() == open(str(tmp_path / "b" / name / f), "rb").read(), f
    assert not os.path.exists(str(tmp_path / "a" / "s_empty"))


def test_a_library_without_the_kernel_is_an_error(oracle):
    from ngspeciesid_amd._capi import NgsidError
    with pytest.raises(NgsidError):
        oracle.demux_locate(ReadSet.from_strings(["ACGT"]), ["AC"])


def test_cli_refusals(tmp_path, caplog):
    from ngspeciesid_amd import cli
    sheet = _sheet(tmp_path, _sheet_text())
    fq = str(tmp_path / "pool.fastq"); open(fq, "w").close()
    d = tmp_path / "in"; d.mkdir()
    base = ["--ont", "--fastq", fq, "--demux_sheet", sheet]
    for argv, text in ((base + ["--outfolder", str(tmp_path / "o"), "--t", "8"], "--demux_sheet requires --t 1"),
                       (base + ["--outfolder", str(tmp_path / "o")], "--demux_sheet requires --t 1"),          # the reference's default --t 8
                       (base + ["--t", "1"], "--demux_sheet needs --outfolder")):
        caplog.clear()
        with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as e:
            cli.cli(argv)
        assert e.value.code not in (0, None) and text in caplog.text
    for argv in (["--ont", "--fastq_dir", str(d), "--demux_sheet", sheet, "--outfolder", str(tmp_path / "o"), "--t", "1"],
                 base + ["--fastq_dir", str(d), "--outfolder", str(tmp_path / "o"), "--t", "1"],
                 ["--ont", "--use_old_sorted_file", "--demux_sheet", sheet, "--outfolder", str(tmp_path / "o"), "--t", "1"]):
        with pytest.raises(SystemExit) as e:
            cli.cli(argv)
        assert e.value.code not in (0, None)
    assert not os.path.exists(str(tmp_path / "o" / "demux"))


def test_header_declares_and_library_exports_the_call():
    text = open(os.path.join(ROOT, "include", "ngsid_demux.h")).read()
    assert '#include "ngsid.h"' in text and re.search(r"int32_t\s+ngsid_demux_locate\s*\(", text)
    assert "ngsid_demux_locate" not in open(os.path.join(ROOT, "include", "ngsid.h")).read()
    from ngspeciesid_amd import runtime
    lib = runtime.load_library()
    assert hasattr(lib, "ngsid_demux_locate") and lib.ngsid_abi_version() == 2
