"""GPU: the alignment statistics on the device (urmapx_bam_stats, urmapx_bam_sort_with; stats.hip) against the host version
(stats_host.cpp) and the model of tests/stats_lib.py, byte for byte: at the edges of the persistent grid, of the LDS copies of the
tables, of the CIGAR sharing and of the staged chunks, beside the sort on both its roads, and through urmapx_map_files."""
import gzip
import os

import numpy as np
import pytest

import bam_lib as bl
import markdup_lib as ml
import stats_lib as st
from test_stats_cpu import ALL_CASES, LENS, NAMES, first_difference, long_cigar_cases, rec

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WAVES = 16                  # stats.h: wavefronts of a workgroup, a record each at a time
L_CYCLES = 160              # cycles whose rows a workgroup counts in LDS
KNOBS = ("URMAPX_TEST_SORT_STAGE", "URMAPX_TEST_SORT_PARTITION", "URMAPX_TEST_SORT_SLICE", "URMAPX_TEST_STATS_BLOCKS", "URMAPX_HOST_TEXT")


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def device_host_model(records, names=NAMES, lens=LENS, model=True):
    """the device's text, held against the host's and (model) the model's -> (text, report)"""
    from urmap_amd import api
    got, rep = api.bam_stats(records, len(lens), names, lens, device=0, report=True)
    want = api.bam_stats_host(records, len(lens), names, lens)
    assert got == want, first_difference(got, want)
    if model:
        want = st.model(records, names, lens)
        assert got == want, first_difference(got, want)
    return got, rep


FLAGS = [0, 0x10, 0x4, 0x63, 0x93, 0x53, 0xa3, 0x400, 0x100, 0x800, 0x463, 0x49, 0x89, 0x200, 0x1, 0x71]
CIGARS = ["", "20M", "5S10M2I3M1D4M", "3M1I3M", "9M70D2M", "4H6M", "2I2D2I2D2I2D2I2D2I2D"]
AUX = [b"", b"NMC\x02", b"ASC\x30XSZhi\0NMc\x07", b"MDZ10A5\0", b"XBBs\x02\0\0\0abcdNMS\x01\x01", b"NMi\xff\xff\xff\xff", b"NM"]


def random_reads(n, seed):
    """n records of every kind in no order: reads of 0 .. 170 bases (some beyond the LDS rows), every flag of FLAGS, tlen to both sides
    of the caps, some without qualities"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        l = int(rng.integers(0, 171)) if rng.random() < 0.9 else int(rng.integers(0, 12))
        qual = rng.integers(0, 60, l).astype(np.uint8)
        if l and rng.random() < 0.05:
            qual[0] = 255
        ref = int(rng.integers(-1, 3))
        out.append(rec(flag=FLAGS[int(rng.integers(0, len(FLAGS)))], ref=ref, pos=int(rng.integers(0, 60000)) if ref >= 0 else -1, mapq=int(rng.integers(0, 61)),
                       next_ref=ref if rng.random() < 0.8 else int(rng.integers(-1, 3)), tlen=int(rng.integers(-600, 9000)), cigar=CIGARS[int(rng.integers(0, len(CIGARS)))],
                       seq=rng.choice([1, 2, 4, 8, 15, 3], l), qual=bytes(qual), aux=AUX[int(rng.integers(0, len(AUX)))]))
    return b"".join(out)


# ---- the persistent grid ----
@pytest.mark.parametrize("n,blocks", [(0, 2), (1, 2), (63, 2), (64, 2), (65, 2), (257, 2), (2 * WAVES + 1, 2), (257, 1), (256 * WAVES + 1, None), (304 * WAVES + 1, None)])
def test_record_counts(monkeypatch, n, blocks):
    """with the grid capped at two workgroups every wavefront loops and both workgroups add their LDS bins to the same tables; the last
    two: one record more than a grid of 256 and of 304 workgroups takes in one round"""
    if blocks:
        monkeypatch.setenv("URMAPX_TEST_STATS_BLOCKS", str(blocks))
    monkeypatch.setenv("URMAPX_TEST_SORT_STAGE", str(1 << 30))  # one chunk: every record in one launch
    records = random_reads(n, n)
    text, rep = device_host_model(records)
    assert rep["records"] == n and rep["stage_chunks"] == (1 if n else 0) and int(st.parse(text)["SN"]["records"]) == n


# ---- the edges of the rule and of the LDS copies ----
@pytest.mark.parametrize("blocks", [None, 1])
@pytest.mark.parametrize("case", list(ALL_CASES))
def test_edge_cases(monkeypatch, case, blocks):
    if blocks:
        monkeypatch.setenv("URMAPX_TEST_STATS_BLOCKS", str(blocks))
    device_host_model(ALL_CASES[case]())


def test_bins_at_both_sides_of_the_lds_caps():
    """cycles 159, 160, 161 on both strands; insert sizes 1023, 1024; read lengths 511, 512; indels of 63 and 64 bases at ops 7 and 8;
    references 1023, 1024 and the row of refID -1 among 1 500 references"""
    names, lens = ["c%d" % k for k in range(1500)], [100 + k for k in range(1500)]
    recs = []
    for l in (L_CYCLES - 1, L_CYCLES, L_CYCLES + 1, 511, 512):
        for flag in (0, 0x10, 0x80, 0x90):
            recs.append(rec(flag=flag, ref=1023, seq=[1, 2, 4, 8, 15] * (l // 5) + [2] * (l % 5), qual=bytes([k % 70 for k in range(l)])))
    for tlen in (1023, 1024, 1025):
        recs.append(rec(flag=0x21, ref=1024, next_ref=1024, tlen=tlen, seq=[1]))
    recs += [rec(ref=r, flag=f, seq=[4]) for r in (0, 1022, 1023, 1024, 1499, -1) for f in (0 if r >= 0 else 4, 0x404)]
    recs.append(rec(ref=3, cigar=[(1, 0)] * 6 + [(63, 1), (63, 2), (64, 1), (64, 2), (63, 1), (63, 2)], seq=[1]))  # ops 6 .. 11: LANE_OPS is 8
    text, rep = device_host_model(b"".join(recs), names, lens)
    t = st.parse(text)
    assert t["IS"] == {1023: (1, 1, 0, 0), 1024: (1, 1, 0, 0), 1025: (1, 1, 0, 0)} and t["ID"] == {63: (2, 2), 64: (1, 1)}
    assert t["RF"][1024] == ("c1024", 1124, 4, 1, 1) and t["RF"][1500] == ("*", 0, 0, 2, 1)


# ---- many atomics on few addresses ----
def test_contention():
    """100 000 copies of one mapped 150-base read: the exact tables are those of one read, times 100 000"""
    n = 100000
    one = rec(flag=0x63, ref=0, pos=100, mapq=37, next_ref=0, tlen=420, cigar="70M2I78M", seq=[1, 2, 4, 8, 2] * 30, qual=bytes([40] * 75 + [11] * 75), aux=b"NMC\x03")
    text, rep = device_host_model(one * n, model=False)
    T = st.count(one, len(LENS))
    for k in T.sn:
        T.sn[k] *= 1 if k == "maximum length" else n
    T.nm_bases, T.qual_sum, T.qual_bases = T.nm_bases * n, T.qual_sum * n, T.qual_bases * n
    T.mq, T.gc = [c * n for c in T.mq], [c * n for c in T.gc]
    for table in ("rl", "isz", "q", "bc", "ind", "rf"):
        setattr(T, table, getattr(T, table) * n)
    want = st.text_of(T, NAMES, LENS)
    assert text == want, first_difference(text, want)
    t = st.parse(text)
    assert t["FFQ"][1][40] == n and t["FFQ"][150][11] == n and len(t["FFQ"]) == 150 and t["BC"][2] == (0, n, 0, 0, 0, 0) and t["IS"] == {420: (n, n, 0, 0)}
    assert t["SN"]["total length"] == str(150 * n) and t["SN"]["average quality"] == "25.50" and t["SN"]["error rate"] == "0.020000"


# ---- CIGAR sharing ----
def test_long_cigars_are_shared_by_the_wavefront():
    device_host_model(long_cigar_cases((8, 9, 64, 65, 65535)) + long_cigar_cases((1, 63, 127, 128, 129)))


# ---- staging ----
def test_staged_chunks_against_one_chunk(monkeypatch):
    records = random_reads(400, 7) + ALL_CASES["aux"]() + ALL_CASES["lengths"]()
    n = len(st.split(records))
    monkeypatch.setenv("URMAPX_TEST_SORT_STAGE", str(1 << 30))
    whole, rep = device_host_model(records)
    assert rep["stage_chunks"] == 1
    for stage, chunks in ((1, lambda c: c == n), (3000, lambda c: 10 < c < n)):
        monkeypatch.setenv("URMAPX_TEST_SORT_STAGE", str(stage))
        text, rep = device_host_model(records, model=False)
        assert text == whole and chunks(rep["stage_chunks"]), rep["stage_chunks"]


# ---- with the sort ----
@pytest.mark.parametrize("depth", [False, True], ids=["alone", "with depth"])
@pytest.mark.parametrize("markdup", [False, True], ids=["plain", "markdup"])
def test_with_the_sort_on_both_roads(monkeypatch, markdup, depth):
    """the statistics' text is the same in core and on the external road, equal to the host sort's and to the model's on the inflated
    stream; the BAM members, the index and the depth are those of the call without stats"""
    from urmap_amd import api
    from test_gpu_depth import many_duplicates
    records, names, lens = many_duplicates()
    records += random_reads(300, 3)
    dep = (names, lens) if depth else None
    texts = {}
    for road in ("in core", "external"):
        if road == "external":
            monkeypatch.setenv("URMAPX_TEST_SORT_SLICE", "1")
            monkeypatch.setenv("URMAPX_TEST_SORT_PARTITION", "1")
            monkeypatch.setenv("URMAPX_TEST_SORT_STAGE", "5000")
        out = api.bam_sort(records, 3, markdup=markdup, budget=0, depth=dep, stats=(names, lens), report=True)
        rep, text = out[-1], out[-2]
        plain = api.bam_sort(records, 3, markdup=markdup, budget=0, depth=dep)
        assert out[:2] == plain[:2], "the statistics changed the file or its index"
        assert not depth or out[2] == plain[2], "the statistics changed the depth"
        assert (rep["external"], rep["partitions"] >= 3) == ((1, True) if road == "external" else (0, False))
        stream = bl.inflate(out[0])
        want = st.model(stream, names, lens)
        assert text == want, first_difference(text, want)
        assert rep["stats_records"] == len(ml.flags_of(stream)) and rep["stats_duplicated"] == int(st.parse(text)["SN"]["reads duplicated"])
        texts[road] = text
    host = api.bam_sort_host(records, 3, markdup=markdup, depth=dep, stats=(names, lens))
    assert texts["in core"] == texts["external"] == host[-1]
    if markdup:  # (the incoming flags give another answer)
        assert texts["in core"] != st.model(records, names, lens) and rep["stats_duplicated"] >= 2 * rep["pairs_duplicate"] > 1000


def test_no_records_through_the_sort():
    from urmap_amd import api
    members, bai, text = api.bam_sort(b"", 3, markdup=True, budget=0, stats=(NAMES, LENS))
    assert text == st.model(b"", NAMES, LENS)


@pytest.mark.parametrize("depth", [False, True], ids=["alone", "with depth"])
def test_a_budget_that_does_not_hold_the_tables_names_the_least(depth):
    from urmap_amd import api
    from test_depth_cpu import duplicated_input
    records, names, lens = duplicated_input()
    n_records = len(st.split(records))
    own = api.bam_stats_resident_bytes(3) + (api.bam_depth_resident_bytes(sum(lens), 3) if depth else 0)
    with pytest.raises(api.UrmapxError) as e:
        api.bam_sort_plan(len(records), n_records, 1, markdup=True)
    least = own + e.value.plan["device_bytes"]
    dep = (names, lens) if depth else None
    for budget in (1000, own - 1, own, least - 1):
        with pytest.raises(api.UrmapxError) as e:
            api.bam_sort(records, 3, markdup=True, budget=budget, depth=dep, stats=(names, lens))
        assert e.value.code == -3 and e.value.least_budget == least and str(least) in str(e.value), (budget, e.value.least_budget, least)
    out = api.bam_sort(records, 3, markdup=True, budget=least, depth=dep, stats=(names, lens))
    assert out[-1] == api.bam_sort_host(records, 3, markdup=True, stats=(names, lens))[-1]


# ---- urmapx_map_files ----
@pytest.fixture(scope="module")
def index(tmp_path_factory):
    from urmap_amd import api
    d = tmp_path_factory.mktemp("stats")
    ufi = os.path.join(d, "g.ufi")
    with gzip.open(os.path.join(GOLD, "g.ufi.gz"), "rb") as z, open(ufi, "wb") as f:
        f.write(z.read())
    return {"dir": str(d), "index": api.Index.open(ufi).upload(0)}


def no_pg(blob):
    """the header of a BAM file without its @PG line, its references, its records"""
    inflated = bl.inflate(blob)
    text, refs, _ = bl.read_bam(inflated)
    return b"\n".join(l for l in text.split(b"\n") if not l.startswith(b"@PG")), refs, inflated[len(bl.bam_header(text, refs)):]


@pytest.mark.parametrize("reads", [("pe150_1.fq", "pe150_2.fq"), ("se150.fq",)], ids=["pe150", "se150"])
def test_map_files(monkeypatch, index, reads):
    """-sort -markdup -stats: the file is the model's for the records the BAM file holds, with the command in its second line; the same
    file under URMAPX_HOST_TEXT=1, with one and two streams and two batch sizes; the BAM file and its index are those of the run without stats_out
    that carries the same command text"""
    from urmap_amd import api
    fq = [os.path.join(GOLD, r) for r in reads]
    path = lambda k, ext: os.path.join(index["dir"], "%s_%s.%s" % (reads[0][:5], k, ext))  # noqa: E731
    common = dict(first_gpu=0, gpus=1, bam=True, bam_sort=True, markdup=True)
    api.map_files(index["index"], *fq, samout=path("plain", "bam"), cmdline="urmap -stats x", **common)
    rep = api.map_files(index["index"], *fq, samout=path("dev", "bam"), cmdline="urmap -stats x", stats_out=path("dev", "stats"), **common)
    hdr, refs, records = no_pg(open(path("dev", "bam"), "rb").read())
    # (the same command text in both @PG lines: nothing else may differ, and the header block in front of the records is as long)
    assert open(path("dev", "bam"), "rb").read() == open(path("plain", "bam"), "rb").read()
    assert open(path("dev", "bam.bai"), "rb").read() == open(path("plain", "bam.bai"), "rb").read()
    want = st.model(records, [n for n, _ in refs], [l for _, l in refs], b"urmap -stats x")
    got = open(path("dev", "stats"), "rb").read()
    assert got == want, first_difference(got, want)
    t = st.parse(got)
    assert int(t["SN"]["reads"]) == rep["reads"] == rep["stats_reads"] > 100 and rep["stats_mapped"] == int(t["SN"]["reads mapped"]) > 100
    assert rep["stats_duplicated"] == int(t["SN"]["reads duplicated"]) == 2 * rep["pairs_duplicate"] + rep["fragments_duplicate"]
    assert rep["stats_insert_median"] == int(t["SN"]["insert size median"]) and (len(reads) == 1 or rep["stats_insert_median"] > 100)
    assert len(t["BC"]) == 150 and rep["stats_s"] > 0
    for k, kw, env in (("host", {}, {"URMAPX_HOST_TEXT": "1"}), ("s1", {"streams": 1, "batch": 64}, {}), ("s2", {"streams": 2, "batch": 1000}, {})):
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        api.map_files(index["index"], *fq, samout=path(k, "bam"), cmdline="urmap -stats x", stats_out=path(k, "stats"), **common, **kw)
        assert open(path(k, "stats"), "rb").read() == want, k
        for name in env:
            monkeypatch.delenv(name)
    # the refusals of the options
    for kw, word in ((dict(bam=True), "stats_out needs bam_sort"), (dict(bam=True, bam_sort=True, stats_out=""), "needs a file name"),
                     (dict(bam=True, bam_sort=True, stats_out=path("no", "bam")), "file of their own"),
                     (dict(bam=True, bam_sort=True, stats_out=path("no", "bam") + ".bai"), "file of their own"),
                     (dict(bam=True, bam_sort=True, depth_out=path("no", "x"), stats_out=path("no", "x")), "file of their own")):
        with pytest.raises(api.UrmapxError) as e:
            api.map_files(index["index"], *fq, samout=path("no", "bam"), **{"stats_out": path("no", "stats"), **kw})
        assert e.value.code == api.E_ARG and word in str(e.value) and not os.path.exists(path("no", "bam")) and not os.path.exists(path("no", "stats"))
