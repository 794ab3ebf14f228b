"""GPU: ngsid_demux_locate (include/ngsid_demux.h, csrc/k_demux.hip) through Api.demux_locate against tests/demux_reference.py over the library's own host locator.
Every comparison is exact equality of hits, ed_all and end_all.  The last test runs `--demux_sheet` of the command line against `--fastq_dir` on sample files the
test wrote itself."""
import os
import numpy as np
import pytest
import demux_reference as ref
from ngspeciesid_amd import runtime, demux
from ngspeciesid_amd._capi import ReadSet, NgsidError

pytestmark = pytest.mark.gpu


def _rand(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def _same(got, want, what):
    for g, w, name in zip(got, want, ("hits", "ed_all", "end_all")):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s: %s differs at %s: got %s, want %s" % (what, name, bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _check(api, reads, tags, window, max_ed, iupac=True, what=""):
    want = ref.locate(reads, tags, window, max_ed, iupac)
    got = api.demux_locate(ReadSet.from_strings(reads), tags, window=window, max_ed=max_ed, iupac=iupac, matrices=True)
    _same(got, want, "%s W=%d max_ed=%d iupac=%d" % (what, window, max_ed, iupac))
    return want


@pytest.mark.parametrize("W", [1, 63, 64, 65, 150, 256])
def test_edges_of_the_bit_vector_step(gpu_api, W):
    """tag lengths around the word halves and the top bit, read lengths around the window, the tag in the first / last column, cut off by the window's end and
    twice at equal distance; max_ed 0, 3 and above every tag length"""
    rng = np.random.default_rng(100 + W)
    base = _rand(rng, 64)
    tags = [base[:m] for m in (1, 2, 31, 32, 33, 63, 64)]
    reads = ["", "A", _rand(rng, max(W - 1, 0)), _rand(rng, W), _rand(rng, W + 1), _rand(rng, 2 * W)]
    twice = {}
    for x, t in enumerate(tags):
        m = len(t)
        reads.append(t + _rand(rng, 2 * W))                                                   # first column
        if W >= m:
            reads.append(_rand(rng, W - m) + t + _rand(rng, W))                               # ends in the last column of the window
            reads.append(_rand(rng, W - m + m // 2) + t + _rand(rng, W))                      # cut off by the window's end
        reads.append(ref.revcomp(t + _rand(rng, 2 * W)))                                      # at the head of side 1
        if W >= 2 * m + 3:
            twice[x] = len(reads)
            reads.append("CA" + t + "G" + t + _rand(rng, W))                                  # twice, exact: the first occurrence
            mut = t[:m // 2] + ("A" if t[m // 2] != "A" else "C") + t[m // 2 + 1:]
            reads.append(mut + "TT" + mut + _rand(rng, W))                                    # twice at distance <= 1
    while len(reads) < 300:
        L = int(rng.integers(0, 2 * W + 40))
        r = _rand(rng, L, "ACGTN" if len(reads) % 7 == 0 else "ACGT")
        if len(reads) % 3 == 0 and L > 70: p = int(rng.integers(0, L - 64)); r = r[:p] + base[:int(rng.integers(1, 65))] + r[p:]
        reads.append(r)
    for max_ed in (0, 3, 64):
        want = _check(gpu_api, reads, tags, W, max_ed, what="edges")
        for x, i in twice.items():
            if len(tags[x]) >= 31:
                assert want[1][i, 0, x] == 0 and want[2][i, 0, x] == 2 + len(tags[x]) - 1              # the first of the two occurrences


@pytest.mark.parametrize("T", [1, 3, 63, 64, 65, 130])
def test_tag_list_passes(gpu_api, T):
    """mixed tag lengths within a wave; the best tag in the last pass; two identical tags in different passes (or lanes): the smaller index wins and ed2 == ed"""
    rng = np.random.default_rng(200 + T)
    tags = [_rand(rng, int(rng.integers(12, 41))) for _ in range(T)]
    twin = None
    if T >= 65:
        twin = (5, T - 3); tags[twin[1]] = tags[twin[0]]                                   # pass 0 and the last pass
    elif T >= 3:
        twin = (0, T - 1); tags[twin[1]] = tags[twin[0]]
    W = 100
    last = T - 1 if (T >= 65 or T == 1) else T - 2
    reads = []
    for i in range(120):
        r = _rand(rng, int(rng.integers(60, 260)))
        if i % 4 == 0: r = _rand(rng, int(rng.integers(0, 20))) + tags[last] + r                            # a tag of the last pass
        if i % 4 == 1 and twin: r = _rand(rng, int(rng.integers(0, 20))) + tags[twin[0]] + r
        if i % 4 == 2: r = ref.revcomp(_rand(rng, 5) + tags[int(rng.integers(0, T))] + r)
        reads.append(r)
    want = _check(gpu_api, reads, tags, W, 3, what="T=%d" % T)
    h = want[0]
    assert (h[0::4, 0, 0] == last).all() and (h[0::4, 0, 1] == 0).all()
    if twin:
        assert (h[1::4, 0, 0] == twin[0]).all() and (h[1::4, 0, 1] == 0).all() and (h[1::4, 0, 4] == 0).all()           # smaller index, ed2 == ed
    _check(gpu_api, reads, tags, W, 40, what="T=%d, every tag hits" % T)


@pytest.mark.parametrize("W", [129, 256])
@pytest.mark.parametrize("T", [1, 2])
def test_lanes_outside_every_group(gpu_api, T, W):
    """windows above 128 bases cap a wave at 32 read-sides: with one tag lanes 32 .. 63 of every wave belong to no group, with two every lane does"""
    rng = np.random.default_rng(500 + 10 * T + W)
    tags = [_rand(rng, m) for m in (30, 64)[:T]]
    reads = []
    for i in range(150):
        r = _rand(rng, int(rng.integers(0, 2 * W + 41)), "ACGTN" if i % 7 == 0 else "ACGT")
        if i % 3 == 0:
            p = int(rng.integers(0, len(r) + 1)); t = tags[int(rng.integers(0, T))]
            r = r[:p] + (t if i % 2 else ref.revcomp(t)) + r[p:]
        reads.append(r)
    want = _check(gpu_api, reads, tags, W, 3, what="T=%d" % T)
    assert (want[0][0::3, :, 0] >= 0).any(axis=1).mean() > 0.5                           # most planted tags lie inside a window


CODES = {"R": "AG", "Y": "CT", "N": "ACGT", "X": "ACGT", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "M": "AC", "K": "GT", "S": "CG", "W": "AT"}


def test_iupac_and_errors(gpu_api):
    rng = np.random.default_rng(300)
    tags = ["ACGTRYACGTAC", "NNACGTTGCANN", "ACBDHVACGTTT", "GGMKSWGGATCC", "ACGTACGTACGT", "XACGTTTGGA"]
    reads = []
    for i in range(150):
        r = _rand(rng, int(rng.integers(40, 200)), "ACGTN" if i % 3 == 0 else "ACGT")
        if i % 2 == 0:
            t = tags[i % len(tags)]
            conc = "".join(CODES.get(c, c)[int(rng.integers(0, len(CODES.get(c, c))))] for c in t)
            r = r[:7] + conc + r[7:]
            if i % 4 == 0: r = r[:9] + "N" + r[10:]                                         # N in the read inside the tag
        reads.append(r)
    on = _check(gpu_api, reads, tags, 150, 2, iupac=True, what="iupac")
    off = _check(gpu_api, reads, tags, 150, 2, iupac=False, what="no iupac")
    assert (on[0][0::2, 0, 0] >= 0).all()                                                   # every concretised tag is found with the equalities ...
    assert not np.array_equal(on[1], off[1]) and (off[1][:, :, :4] >= 0).sum() < (on[1][:, :, :4] >= 0).sum()      # ... and mostly not without them
    rs = ReadSet.from_strings(["ACGTACGTAC", "ACGTaCGTAC"])
    for kw, code in ((dict(tags=["ACGT"]), -3), (dict(tags=["A" * 65]), -6), (dict(tags=[]), -2), (dict(tags=["ACGT"], window=0), -2),
                     (dict(tags=["ACGT"], window=257), -2), (dict(tags=["ACGT"], max_ed=-1), -2)):
        with pytest.raises(NgsidError) as e:
            gpu_api.demux_locate(rs, **kw)
        assert e.value.code == code, kw
    empty_tag = ReadSet(np.frombuffer(b"ACGT", dtype=np.uint8), None, np.array([0, 4, 4], dtype=np.uint64))
    with pytest.raises(NgsidError) as e:
        gpu_api.demux_locate(rs, empty_tag)
    assert e.value.code == -2
    assert gpu_api.demux_locate(ReadSet.from_strings([]), ["ACGT"]).shape == (0, 2, 5)        # an empty read set is legal
    assert gpu_api.demux_locate(ReadSet.from_strings(["ACGTACGTAC"]), ["A" * 64]).tolist() == [[[-1] * 5, [-1] * 5]]


def test_host_and_device_reads_and_chunking():
    rng = np.random.default_rng(400)
    tags = [_rand(rng, 24) for _ in range(96)]
    reads = []
    for i in range(5000):
        a = _rand(rng, int(rng.integers(150, 420)))
        f, r = tags[int(rng.integers(0, 96))], tags[int(rng.integers(0, 96))]
        if i % 5: a = _rand(rng, int(rng.integers(0, 25))) + f + a + ref.revcomp(r)
        reads.append(a)
    rs = ReadSet.from_strings(reads)
    with runtime.new_api() as api:
        plain = api.demux_locate(rs, tags, window=150, max_ed=3)
        full = api.demux_locate(rs, tags, window=150, max_ed=3, matrices=True)
        dev = api.upload_reads(rs)
        try:
            on_dev = api.demux_locate(dev, tags, window=150, max_ed=3)
            api.set_option("demux_chunk_reads", 700)                                         # 8 chunks, the last one short
            chunked = api.demux_locate(dev, tags, window=150, max_ed=3, matrices=True)
            chunked_plain = api.demux_locate(rs, tags, window=150, max_ed=3)
            api.set_option("demux_chunk_reads", 0)
        finally:
            dev.release()
    assert np.array_equal(plain, full[0]) and np.array_equal(plain, on_dev) and np.array_equal(plain, chunked_plain)
    _same(chunked, full, "chunked vs one launch")
    sub = list(range(0, 5000, 10))
    want = ref.locate([reads[i] for i in sub], tags, 150, 3)
    _same([x[sub] for x in full], want, "every tenth read against the reference")
    assert (plain[:, :, 0] >= 0).mean() > 0.6


# ---- the command line
def _files(folder):
    out = {}
    for root, _, fs in os.walk(folder):
        for f in fs:
            out[os.path.relpath(os.path.join(root, f), folder)] = open(os.path.join(root, f), "rb").read()
    return out


def test_cli_demux_sheet_equals_fastq_dir_on_the_reference_split(gpu_api, tmp_path):
    from ngspeciesid_amd.cli import cli
    tags = ref.make_tags(8, 24, 9, seed=5)
    fwd, rev = tags[0::2], tags[1::2]
    names = ["s_one", "s_two", "s_three", "s_empty"]
    pool = ref.make_pool(fwd, rev, 150, seed=9, n_species=2, length=420, junk_reads=8, mu=18.0, samples=[0, 1, 2])
    fq = str(tmp_path / "pool.fastq"); ref.write_fastq(fq, pool["names"], pool["seqs"], pool["quals"])
    sheet_path = str(tmp_path / "sheet.tsv")
    open(sheet_path, "w").write("#sample\tforward\treverse\n" + "".join("%s\t%s\t%s\n" % x for x in zip(names, fwd, rev)))
    flags = ["--t", "1", "--consensus", "--racon", "--racon_iter", "2"]
    # run A
    cli(["--ont", "--fastq", fq, "--outfolder", str(tmp_path / "A"), "--demux_sheet", sheet_path] + flags)
    # run B: the split by the reference + assign(), written by the test, through --fastq_dir
    sheet = demux.read_sheet(sheet_path)
    hits = ref.locate(pool["seqs"], sheet.tags, 150, 3, True)[0]
    sample, strand, status, c0, c1 = demux.assign(hits, sheet, 2, lens=np.array([len(s) for s in pool["seqs"]]))
    good = ~pool["junk"] & (pool["edits"].max(axis=1) <= 3)
    assert (status[good] == 0).all() and np.array_equal(sample[good], pool["sample"][good]) and (status[pool["junk"]] == 1).all()
    d = tmp_path / "split"; d.mkdir()
    for s in range(3):
        idx = np.flatnonzero(sample == s)
        assert len(idx) >= 100
        ref.write_fastq(str(d / (names[s] + ".fastq")), [pool["names"][i] for i in idx], [pool["seqs"][i][c0[i]:len(pool["seqs"][i]) - c1[i]] for i in idx],
                        [pool["quals"][i][c0[i]:len(pool["seqs"][i]) - c1[i]] for i in idx])
    cli(["--ont", "--fastq_dir", str(d), "--outfolder", str(tmp_path / "B")] + flags)
    got, want = _files(str(tmp_path / "A")), _files(str(tmp_path / "B"))
    assert sorted(k for k in got if not k.startswith("demux")) == sorted(want)
    for k in want:
        assert got[k] == want[k], k
    for s in range(3):
        assert got["demux/%s.fastq" % names[s]] == open(str(d / (names[s] + ".fastq")), "rb").read()
        assert any(k.startswith(names[s] + "/racon_cl_id_") for k in got) and names[s] + "/final_clusters.tsv" in got
    assert "demux/s_empty.fastq" not in got and not any(k.startswith("s_empty/") for k in got)
    rows = {l.split("\t")[0]: l.split("\t")[1:] for l in got["demux_summary.tsv"].decode().splitlines()}
    assert rows["s_empty"] == ["0", "0", "0", "0"] and int(rows["s_one"][0]) == int((sample == 0).sum())
    un = got["demux_unassigned.fastq"].decode().split("\n")
    assert un[0::4][:-1] == ["@" + pool["names"][i] for i in np.flatnonzero(sample < 0)]
    # --demux_only stops after the three outputs
    cli(["--ont", "--fastq", fq, "--outfolder", str(tmp_path / "C"), "--demux_sheet", sheet_path, "--demux_only"] + flags)
    only = _files(str(tmp_path / "C"))
    assert sorted(only) == sorted(k for k in got if k.startswith("demux")) and all(only[k] == got[k] for k in only)
