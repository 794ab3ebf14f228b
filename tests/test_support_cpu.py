"""CPU: the definition of the per-base consensus support (tests/support_reference.py, built from the oracle's parts) on hand-derived vectors, the quality formula, the
writers of --consensus_support and the flag itself with a stubbed consensus_support (the oracle has no such entry point: the HIP library is checked against the same
definition in tests/test_gpu_support.py)."""
import os, shutil, tempfile
import numpy as np
import pytest
from oracle_lib import GOLD
from ngspeciesid_amd import cli, consensus, fastpath
from ngspeciesid_amd._capi import ReadSet, NgsidError
from support_reference import support_reference, _COMP

K, W = 7, 7
# 72 bases, no base equal to its neighbour: every edit below has ONE optimal placement
CENTRE = "ACGTCAGTACTGCATGACGTAGCTAGTCGATCGTACGATGCTAGCATCGTGACTGATCGCATGCTGACTAGC"
OTHER = "AG" * 32             # shares no 7-mer with CENTRE, in either orientation


def _rc(s):
    return _COMP[np.frombuffer(s.encode(), dtype=np.uint8)[::-1]].tobytes().decode()


def _perfect(n):
    e = np.zeros((len(CENTRE), 8), dtype=np.uint32); e[:, 0] = n; e[:, 1] = n
    return e


def _run(oracle, reads, clip=False, centre=CENTRE):
    rs = ReadSet.from_strings(reads)
    return support_reference(oracle, [centre], rs, [0, len(reads)], None, K, W, clip)


def test_centre_has_no_equal_neighbours():
    assert all(a != b for a, b in zip(CENTRE, CENTRE[1:])) and len(CENTRE) == 72


def _foreign(i):
    """a letter that differs from base i of the centre and from both its neighbours"""
    return next(c for c in "ACGT" if c not in CENTRE[max(i - 1, 0):i + 2])


def test_hand_vectors(oracle):
    sl = _foreign(30); sub = CENTRE[:30] + sl + CENTRE[31:]                               # a substitution at base 30
    dele = CENTRE[:40] + CENTRE[41:]                                                      # base 40 missing
    il = next(c for c in "ACGT" if c not in CENTRE[50:52]); ins = CENTRE[:51] + il + il + CENTRE[51:]      # two bases behind base 50
    withn = CENTRE[:10] + "N" + CENTRE[11:]
    reads = [CENTRE, sub, dele, ins, _rc(CENTRE), withn, OTHER]
    counts, cen_off, used, strand = _run(oracle, reads)
    assert strand.tolist() == [0, 0, 0, 0, 1, 0, -1]
    assert used.tolist() == [6] and cen_off.tolist() == [0, 72]
    e = _perfect(6)
    e[30, 1] -= 1; e[30, 2 + "ACGT".index(sl)] += 1      # sub_<letter>
    e[40, 1] -= 1; e[40, 6] += 1                 # del
    e[50, 7] += 1                                # one run of two inserted bases, counted once
    e[10, 1] -= 1                                # N in the read: depth only
    assert np.array_equal(counts, e)
    assert (counts[:, 0] >= counts[:, 1:7].sum(axis=1)).all()


def test_overhanging_and_partial_reads(oracle):
    over = "GGTTGGTT" + CENTRE + "TTGGTTGG"          # overhangs both centre ends: the overhang is read-only columns outside the counted ones
    part = CENTRE[20:60]
    counts, _, used, strand = _run(oracle, [over, part])
    e = np.zeros((72, 8), dtype=np.uint32); e[:, 0:2] = 1; e[20:60, 0:2] += 1
    assert np.array_equal(counts, e) and used.tolist() == [2] and strand.tolist() == [0, 0]


def test_clip_counts_between_runs_of_15_only(oracle):
    # a primer-like overhang that happens to end in the centre's first base, then a substitution at base 5: without clipping the columns 0 .. 71 count, with it the
    # columns from the first run of 15 equal ones (bases 6 .. 71)
    r = "GGTTGGTT" + CENTRE[:5] + _foreign(5) + CENTRE[6:]
    c0, _, u0, _ = _run(oracle, [r], clip=False)
    c1, _, u1, _ = _run(oracle, [r], clip=True)
    assert c0[:, 0].tolist() == [1] * 72 and c0[5, 1] == 0 and c0[:, 1].sum() == 71
    assert c1[:6].sum() == 0 and c1[6:, 0].tolist() == [1] * 66 and c1[6:, 1].tolist() == [1] * 66
    short = CENTRE[:10] + _foreign(10) + CENTRE[11:22]                         # no run of 15: contributes nothing when clipped
    c2, _, u2, _ = _run(oracle, [short], clip=True)
    assert c2.sum() == 0 and u2.tolist() == [0] and u0.tolist() == [1] and u1.tolist() == [1]


def test_empty_and_unrelated_groups(oracle):
    rs = ReadSet.from_strings([OTHER, CENTRE])
    counts, cen_off, used, strand = support_reference(oracle, [CENTRE, CENTRE, CENTRE], rs, [0, 0, 1, 2], None, K, W, False)
    assert used.tolist() == [0, 0, 1] and strand.tolist() == [-1, 0]
    assert counts[:144].sum() == 0 and np.array_equal(counts[144:], _perfect(1))


def test_support_phred_hand_values():
    # (depth - agree + 1) / (depth + 2): 1/12 -> 10.79, 3/12 -> 6.02, 1/3 -> 4.77, 11/12 -> 0.38, 1/2002 -> 33.01; depth 0 -> 0; 60 is the cap
    c = np.zeros((7, 8), dtype=np.uint32)
    c[:, 0] = [10, 10, 1, 10, 2000, 0, 4_000_000]; c[:, 1] = [10, 8, 1, 0, 2000, 0, 4_000_000]
    assert consensus.support_phred(c).tolist() == [10, 6, 4, 0, 33, 0, 60]


def test_writers(tmp_path):
    c = np.zeros((4, 8), dtype=np.uint32); c[:, 0] = [10, 10, 0, 10]; c[:, 1] = [10, 8, 0, 0]; c[1, 3] = 2; c[3, 6] = 10; c[0, 7] = 1
    fa = tmp_path / "consensus.fasta"; fa.write_text(">name LN:i:4 RC:i:10 XC:f:1.000000\nACGT\n")
    consensus.write_support_for_fasta(str(fa), str(tmp_path / "c.fastq"), str(tmp_path / "c.tsv"), c)
    assert (tmp_path / "c.fastq").read_text() == "@name LN:i:4 RC:i:10 XC:f:1.000000\nACGT\n+\n" + "".join(chr(33 + q) for q in (10, 6, 0, 0)) + "\n"
    assert (tmp_path / "c.tsv").read_text().splitlines() == ["pos\tbase\tdepth\tagree\tA\tC\tG\tT\tdel\tins_after", "1\tA\t10\t10\t0\t0\t0\t0\t0\t1", "2\tC\t10\t8\t0\t2\t0\t0\t0\t0",
                                                             "3\tG\t0\t0\t0\t0\t0\t0\t0\t0", "4\tT\t10\t0\t0\t0\t0\t0\t10\t0"]
    with pytest.raises(ValueError):
        consensus.write_support_files(str(tmp_path / "x.fastq"), str(tmp_path / "x.tsv"), "n", "ACG", c)


def test_flag_parsing():
    base = ["--ont", "--fastq", "x.fastq", "--outfolder", "o"]
    assert cli.build_parser().parse_args(base).consensus_support is False
    assert cli.build_parser().parse_args(base + ["--consensus_support"]).consensus_support is True


def test_binding_without_the_symbol_is_an_error(oracle):
    rs = ReadSet.from_strings([CENTRE])
    with pytest.raises(NgsidError, match="consensus_support"):
        oracle.consensus_support(ReadSet.from_strings([CENTRE]), rs, [0, 1])


def _cli_files(api, extra):
    out = tempfile.mkdtemp()
    args = cli.build_parser().parse_args(["--ont", "--fastq", os.path.join(GOLD, "sample_h1.fastq"), "--outfolder", out, "--t", "1", "--consensus"] + extra)
    args.k, args.w = 13, 20
    fastpath.main(args, api=api)
    files = {}
    for root, _, fs in os.walk(out):
        for f in fs:
            files[os.path.relpath(os.path.join(root, f), out)] = open(os.path.join(root, f), "rb").read()
    shutil.rmtree(out)
    return files


@pytest.mark.parametrize("extra", [["--racon", "--racon_iter", "1"], []])
def test_cli_flag_adds_files_and_changes_no_other(oracle, monkeypatch, extra):
    """the flag with consensus_support stubbed by the reference definition: the files of a run without it, unchanged, plus the two new ones per centre"""
    calls = []
    def stub(centres, rs, grp_off, read_order=None, k=13, w=20, clip=False):
        calls.append(clip)
        cs = [centres.get(i)[0] for i in range(centres.n)]
        return support_reference(oracle, cs, rs, grp_off, read_order, k, w, clip)
    monkeypatch.setattr(oracle, "consensus_support", stub, raising=False)
    a = _cli_files(oracle, extra); assert not calls
    b = _cli_files(oracle, extra + ["--consensus_support"]); assert calls == [False]
    new = sorted(set(b) - set(a))
    assert set(a) <= set(b) and all(a[f] == b[f] for f in a)
    if extra:
        folders = sorted({os.path.dirname(f) for f in a if f.endswith("consensus.fasta")})
        assert folders and new == sorted(os.path.join(d, n) for d in folders for n in ("consensus.fastq", "consensus_support.tsv"))
        pairs = [(os.path.join(d, "consensus.fasta"), os.path.join(d, "consensus.fastq"), os.path.join(d, "consensus_support.tsv")) for d in folders]
    else:
        refs = sorted(f[:-len(".fasta")] for f in a if f.startswith("consensus_reference_"))
        assert refs and new == sorted(r + s for r in refs for s in (".fastq", ".support.tsv"))
        pairs = [(r + ".fasta", r + ".fastq", r + ".support.tsv") for r in refs]
    for fa, fq, tsv in pairs:
        fal = b[fa].decode().split("\n"); fql = b[fq].decode().split("\n"); rows = b[tsv].decode().splitlines()
        assert fql[0] == "@" + fal[0][1:] and fql[1] == fal[1] and fql[2] == "+" and len(fql[3]) == len(fal[1])
        assert len(rows) == len(fal[1]) + 1 and "".join(r.split("\t")[1] for r in rows[1:]) == fal[1]
        depth = np.array([int(r.split("\t")[2]) for r in rows[1:]]); assert depth.max() > 10
