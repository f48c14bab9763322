"""GPU: the pileup on the device (urmapx_bam_pileup, urmapx_bam_sort_with; pileup.hip) against the host version (pileup_host.cpp)
and the model of tests/pileup_lib.py, byte for byte: at the edges of the persistent grid, of the 64 lanes and the nibbles, of the CIGAR
sharing, of the references, of the segments and slices of the site search, with counter offsets past 2^32 bytes, beside the sort on
both its roads, and through urmapx_map_files.  Columns beyond 2^32 are not tested: their counters alone would take 64 GiB."""
import gzip
import os

import numpy as np
import pytest

import bam_lib as bl
import depth_lib as dl
import pileup_lib as pl
from stats_lib import parse_cigar, rec
from test_pileup_cpu import (ANY, LENS, NAMES, SEQS, cigar_cases, column_with, edge_cases, filter_cases, first_difference, lane_cases, letter_cases, matching, other,
                             sort_input)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WAVES = 4                   # pileup.h: wavefronts of a workgroup, a record each at a time
KNOBS = ("URMAPX_TEST_SORT_STAGE", "URMAPX_TEST_SORT_PARTITION", "URMAPX_TEST_SORT_SLICE", "URMAPX_TEST_PILEUP_BLOCKS", "URMAPX_TEST_PILEUP_SEGMENT",
         "URMAPX_TEST_PILEUP_SLICE", "URMAPX_HOST_TEXT", "URMAPX_HOST_INDEX")


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def device_host_model(records, opts=None, names=NAMES, lens=LENS, seqs=SEQS, model=True):
    """the device's text, held against the host's and (model) the model's -> (parsed text, report)"""
    from urmap_amd import api
    got, rep = api.bam_pileup(records, len(lens), names, lens, seqs, opts=opts, device=0, report=True)
    want, hrep = api.bam_pileup_host(records, len(lens), names, lens, seqs, opts=opts, report=True)
    assert got == want, first_difference(got, want)
    assert [rep[k] for k in ("sites", "alt_alleles", "records")] == [hrep[k] for k in ("sites", "alt_alleles", "records")]
    if model:
        want = pl.model(records, names, lens, seqs, opts)
        assert got == want, first_difference(got, want)
    return pl.parse(got), rep


CIGARS = ["150M", "20M", "5S10M2I3M1D4M", "3M1I3M", "9M70D2M", "4H6M", "2I2D2I2D2I2D2I2D2I2D", "70M30N70M", "1S148M1S"]


def random_reads(n, seed):
    """n records of every kind in no order: with and without a reference, flags that count and that do not, bases of every code"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        cigar = CIGARS[int(rng.integers(0, len(CIGARS)))]
        l = sum(length for length, op in parse_cigar(cigar) if op in (0, 1, 4, 7, 8)) if rng.random() < 0.95 else int(rng.integers(0, 12))
        qual = rng.integers(0, 45, l).astype(np.uint8)
        if l and rng.random() < 0.05:
            qual[0] = 255
        ref = int(rng.choice([-1, 0, 1, 2, 3, 3, 3]))
        top = max(1, LENS[ref]) if ref >= 0 else 1
        out.append(rec(flag=int(rng.choice([0, 0x10, 0x4, 0x63, 0x93, 0x400, 0x100, 0x800, 0x200, 0x1])), ref=ref, pos=int(rng.integers(0, top + 20)) % 2000 if ref >= 0 else -1,
                       mapq=int(rng.integers(0, 61)), cigar=cigar, seq=rng.choice([1, 2, 4, 8, 15, 3], l), qual=bytes(qual), name=b"q" * int(rng.integers(1, 9))))
    return b"".join(out)


# ---- 1. the persistent grid ----
@pytest.mark.parametrize("n,blocks", [(0, 2), (1, 2), (63, 2), (64, 2), (65, 2), (2 * 2 * WAVES + 1, 2), (0, 1), (1, 1), (63, 1), (64, 1), (65, 1), (2 * WAVES + 1, 1)])
def test_record_counts(monkeypatch, n, blocks):
    """with the grid capped at one and at two workgroups every wavefront loops, and both workgroups add to the same columns"""
    monkeypatch.setenv("URMAPX_TEST_PILEUP_BLOCKS", str(blocks))
    monkeypatch.setenv("URMAPX_TEST_SORT_STAGE", str(1 << 30))  # one chunk: every record in one launch
    t, rep = device_host_model(random_reads(n, 100 + n), ANY)
    assert rep["stage_chunks"] == (1 if n else 0) and (n < 63 or len(t["sites"]) > 50)


# ---- 2 .. 7. the edges of the rule ----
CASES = {"lanes": (lane_cases, [None, ANY, {"min_baseq": 0, "min_alt": 1}]), "cigars": (cigar_cases, [ANY, {"min_baseq": 20, "min_alt": 2, "min_pct": 30}]),
         "edges": (edge_cases, [ANY]), "filters": (filter_cases, [dict(ANY, min_mapq=20), None]), "letters": (letter_cases, [ANY, None])}


@pytest.mark.parametrize("blocks", [None, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_edge_cases(monkeypatch, case, blocks):
    if blocks:
        monkeypatch.setenv("URMAPX_TEST_PILEUP_BLOCKS", str(blocks))
    make, all_opts = CASES[case]
    for opts in all_opts:
        t, rep = device_host_model(make(), opts)
    if case == "letters":
        assert not any(c == "chrA" and (96 <= p <= 115 or 201 <= p <= 210) for c, p, *_ in t["sites"])


def test_fifteen_hundred_references():
    rng = np.random.default_rng(2)
    names, lens = ["c%d" % k for k in range(1500)], [(k * 7) % 40 for k in range(1500)]
    seqs = [rng.choice(list(b"ACGT"), l).astype(np.uint8).tobytes() for l in lens]
    recs = b"".join(rec(ref=r, pos=0, cigar="50M", seq=rng.choice([1, 2, 4, 8], 50)) for r in range(0, 1500, 3))
    t, rep = device_host_model(recs, ANY, names, lens, seqs)
    assert len({c for c, *_ in t["sites"]}) > 400 and rep["records"] == 500


def test_the_site_rule_at_its_thresholds():
    t, _ = device_host_model(column_with(1000, 5, [2]) + column_with(1001, 5, [3]), {"min_pct": 0})
    assert [p for _, p, *_ in t["sites"]] == [1002]
    t, _ = device_host_model(column_with(1000, 27, [3]) + column_with(1001, 28, [3]))
    assert [(p, dp, ad) for _, p, _, _, dp, ad in t["sites"]] == [(1001, 30, [27, 3])]
    t, _ = device_host_model(column_with(1000, 4, [3, 5]) + column_with(1001, 1, [4, 6, 5]) + column_with(1002, 0, [4, 4]) + column_with(1003, 2, [3, 3, 3]))
    assert [ad[1:] for *_, ad in t["sites"]] == [[5, 3], [6, 5, 4], [4, 4], [3, 3, 3]]
    both = column_with(1000, 500, [1]) + column_with(1001, 0, [4]) + column_with(1002, 1, [400])
    assert [p for _, p, *_ in device_host_model(both, {"min_alt": 1, "min_pct": 0})[0]["sites"]] == [1001, 1002, 1003]
    assert [p for _, p, *_ in device_host_model(both, {"min_alt": 1, "min_pct": 100})[0]["sites"]] == [1002]


# ---- 8. many atomics on few addresses ----
def test_contention():
    """100 000 copies of one 150-base read with three mismatches: the counts are one read's, times 100 000"""
    n = 100000
    seq = matching(3, 5000, 150)
    for at in (0, 77, 149):
        seq[at] = other([seq[at]])[0]
    one = rec(ref=3, pos=5000, mapq=37, cigar="150M", seq=seq, qual=bytes([40] * 150))
    t, rep = device_host_model(one * n, model=False)
    cnt, counted = pl.counts(one, LENS)
    want = pl.text_of(cnt * n, NAMES, LENS, SEQS)
    assert [(p, dp, ad) for _, p, _, _, dp, ad in t["sites"]] == [(5001, n, [0, n]), (5078, n, [0, n]), (5150, n, [0, n])]
    assert t == pl.parse(want) and rep["records"] == n * counted


# ---- 9. segments and slices ----
def test_segments_and_slices(monkeypatch):
    """segments of 256 columns, slices of 100 entries: sites on the last column of a segment and the first of the next, a segment
    with none, a segment where every column is a site (more than two slices hold)"""
    monkeypatch.setenv("URMAPX_TEST_PILEUP_SEGMENT", "256")
    monkeypatch.setenv("URMAPX_TEST_PILEUP_SLICE", "100")
    recs = [rec(ref=0, pos=254, cigar="4M", seq=other(matching(0, 254, 4)))]                 # columns 254 .. 257: both sides of a segment's edge
    recs += [rec(ref=0, pos=1024, cigar="256M", seq=other(matching(0, 1024, 256)))]          # the whole of segment 4
    recs += [rec(ref=0, pos=2040, cigar="20M", seq=matching(0, 2040, 20))]                   # covered, no site
    recs += [rec(ref=3, pos=4700 + k * 251, cigar="3M", seq=other(matching(3, 4700 + k * 251, 3))) for k in range(40)]
    t, rep = device_host_model(b"".join(recs), ANY)
    cols = [(c, p) for c, p, *_ in t["sites"]]
    assert cols[:4] == [("chrA", p) for p in (255, 256, 257, 258)] and [p for c, p in cols if c == "chrA"][4:] == list(range(1025, 1281))
    monkeypatch.setenv("URMAPX_TEST_PILEUP_SLICE", "1")
    device_host_model(b"".join(recs[:2]), ANY, model=False)


# ---- 10. counter offsets past 2^32 bytes ----
def test_counter_offsets_past_4_gib():
    """references of 2^28 and 4 096 columns (4 GiB and 64 KiB of counters), reads on the last columns of each; device against host
    only (the model's counters would be 8 GiB of int64)"""
    from urmap_amd import api
    big = 1 << 28
    names, lens = ["big", "small"], [big, 4096]
    rng = np.random.default_rng(4)
    tail = rng.choice(list(b"ACGT"), 4096).astype(np.uint8).tobytes()
    seqs = [b"A" * (big - 4096) + tail, tail[::-1]]
    code = {65: 1, 67: 2, 71: 4, 84: 8}
    recs = []
    for k, (ref, pos) in enumerate([(0, big - 150), (0, big - 100), (0, big - 1), (0, big - 70), (1, 0), (1, 4096 - 150), (1, 4095), (0, 0)]):
        span = seqs[ref][pos:pos + 150]
        recs.append(rec(ref=ref, pos=pos, cigar="150M", seq=other([code[b] for b in span] + [1] * (150 - len(span)), 1 + k % 3)))
    got = api.bam_pileup(b"".join(recs), 2, names, lens, seqs, opts=ANY, device=0)
    want = api.bam_pileup_host(b"".join(recs), 2, names, lens, seqs, opts=ANY)
    assert got == want, first_difference(got, want)
    cols = [(c, p) for c, p, *_ in pl.parse(got)["sites"]]
    assert ("big", big) in cols and ("small", 1) in cols and ("small", 4096) in cols and ("big", 1) in cols and len(cols) == 4 * 150


# ---- 11. with the sort ----
def depth_of(text):
    depth = {}
    for name, beg, end, d in dl.parse(text):
        depth.setdefault(name.decode(), []).append((beg, end, d))
    return depth


@pytest.mark.parametrize("beside", [False, True], ids=["alone", "with depth and stats"])
@pytest.mark.parametrize("markdup", [False, True], ids=["plain", "markdup"])
def test_with_the_sort_on_both_roads(monkeypatch, markdup, beside):
    """the VCF text is the same in core and on the external road, equal to the host pileup's and the model's on the inflated sorted,
    marked stream; the BAM members, the index, the depth and the statistics are those of the call without the pileup; at min_baseq 0
    on reads without N every site's DP is the depth file's value"""
    from urmap_amd import api
    from test_gpu_depth import many_duplicates
    records, names, lens = many_duplicates()
    rng = np.random.default_rng(8)
    seqs = [rng.choice(list(b"ACGT"), l).astype(np.uint8).tobytes() for l in lens]
    opts = {"min_baseq": 0, "min_alt": 1, "min_pct": 0}
    dep, sta = ((names, lens), (names, lens)) if beside else (None, None)
    texts = {}
    for road in ("in core", "external"):
        if road == "external":
            monkeypatch.setenv("URMAPX_TEST_SORT_SLICE", "1")
            monkeypatch.setenv("URMAPX_TEST_SORT_PARTITION", "1")
            monkeypatch.setenv("URMAPX_TEST_SORT_STAGE", "5000")
        out = api.bam_sort(records, 3, markdup=markdup, budget=0, depth=dep, stats=sta, pileup=(names, lens, seqs, opts), report=True)
        rep, vcf = out[-1], out[-2]
        plain = api.bam_sort(records, 3, markdup=markdup, budget=0, depth=dep, stats=sta) if beside else api.bam_sort(records, 3, markdup=markdup, budget=0)
        assert out[:len(plain)] == plain, "the pileup changed the file, its index, the depth or the statistics"
        assert (rep["external"], rep["partitions"] >= 3) == ((1, True) if road == "external" else (0, False))
        stream = bl.inflate(out[0])
        want = pl.model(stream, names, lens, seqs, opts)
        assert vcf == want, first_difference(vcf, want)
        assert vcf == api.bam_pileup_host(stream, 3, names, lens, seqs, opts=opts)
        t = pl.parse(vcf)
        assert rep["pileup_sites"] == len(t["sites"]) > 1000
        if beside:
            depth = depth_of(out[2][0])
            for chrom, pos, _, _, dp, _ in t["sites"][::7]:
                assert [d for b, e, d in depth[chrom] if b <= pos - 1 < e] == [dp]
        texts[road] = vcf
    host = api.bam_sort_host(records, 3, markdup=markdup, depth=dep, stats=sta, pileup=(names, lens, seqs, opts))
    assert texts["in core"] == texts["external"] == host[-1]
    if markdup:  # (the incoming flags give another answer)
        assert texts["in core"] != pl.model(records, names, lens, seqs, opts)


def test_no_records_through_the_sort():
    from urmap_amd import api
    members, bai, vcf = api.bam_sort(b"", 4, markdup=True, budget=0, pileup=(NAMES, LENS, SEQS, None))
    assert vcf == pl.model(b"", NAMES, LENS, SEQS)


@pytest.mark.parametrize("beside", [False, True], ids=["alone", "with depth and stats"])
def test_a_budget_that_does_not_hold_the_counters_names_the_least(beside):
    from urmap_amd import api
    records, names, lens, seqs = sort_input()
    n_records = len(pl.split(records))
    own = api.bam_pileup_resident_bytes(sum(lens), 3) + (api.bam_depth_resident_bytes(sum(lens), 3) + api.bam_stats_resident_bytes(3) if beside else 0)
    with pytest.raises(api.UrmapxError) as e:
        api.bam_sort_plan(len(records), n_records, 1, markdup=True)
    least = own + e.value.plan["device_bytes"]
    dep, sta = ((names, lens), (names, lens)) if beside else (None, None)
    for budget in (1000, own - 1, own, least - 1):
        with pytest.raises(api.UrmapxError) as e:
            api.bam_sort(records, 3, markdup=True, budget=budget, depth=dep, stats=sta, pileup=(names, lens, seqs, ANY))
        assert e.value.code == -3 and e.value.least_budget == least and str(least) in str(e.value), (budget, e.value.least_budget, least)
    out = api.bam_sort(records, 3, markdup=True, budget=least, depth=dep, stats=sta, pileup=(names, lens, seqs, ANY))
    assert out[-1] == api.bam_sort_host(records, 3, markdup=True, pileup=(names, lens, seqs, ANY))[-1]


# ---- 12. urmapx_map_files ----
@pytest.fixture(scope="module")
def index(tmp_path_factory):
    from urmap_amd import api
    d = tmp_path_factory.mktemp("pileup")
    ufi = os.path.join(d, "g.ufi")
    with gzip.open(os.path.join(GOLD, "g.ufi.gz"), "rb") as z, open(ufi, "wb") as f:
        f.write(z.read())
    return {"dir": str(d), "ufi": ufi, "index": api.Index.open(ufi).upload(0)}


def fasta(path):
    """{the first word of every header line: its letters}"""
    out, name = {}, None
    for line in open(path, "rb").read().split(b"\n"):
        if line.startswith(b">"):
            name = line[1:].split()[0].decode()
            out[name] = b""
        elif name is not None:
            out[name] += line.strip()
    return out


def records_of(path):
    inflated = bl.inflate(open(path, "rb").read())
    text, refs, _ = bl.read_bam(inflated)
    return refs, inflated[len(bl.bam_header(text, refs)):]


@pytest.mark.parametrize("reads", [("pe150_1.fq", "pe150_2.fq"), ("se150.fq",)], ids=["pe150", "se150"])
def test_map_files(monkeypatch, index, reads):
    """-sort -markdup -vcfout: the file is the model's for the records the BAM file holds and the letters of g.fa, with the command in
    its header; the same file under URMAPX_HOST_TEXT=1 and with two streams and a small batch; the BAM file and its index are those of
    the run without vcf_out that carries the same command text.  Every base that differs (min_alt 1, min_pct 0), then the defaults"""
    from urmap_amd import api
    fq = [os.path.join(GOLD, r) for r in reads]
    path = lambda k, ext: os.path.join(index["dir"], "%s_%s.%s" % (reads[0][:5], k, ext))  # noqa: E731
    common = dict(first_gpu=0, gpus=1, bam=True, bam_sort=True, markdup=True, cmdline="urmap -vcfout x")
    loose = dict(vcf_min_alt=1, vcf_min_pct=0)
    api.map_files(index["index"], *fq, samout=path("plain", "bam"), **common)
    rep = api.map_files(index["index"], *fq, samout=path("dev", "bam"), vcf_out=path("dev", "vcf"), **common, **loose)
    assert open(path("dev", "bam"), "rb").read() == open(path("plain", "bam"), "rb").read()
    assert open(path("dev", "bam.bai"), "rb").read() == open(path("plain", "bam.bai"), "rb").read()
    refs, records = records_of(path("dev", "bam"))
    letters = fasta(os.path.join(GOLD, "g.fa"))
    names, lens = [n.decode() if isinstance(n, bytes) else n for n, _ in refs], [l for _, l in refs]
    seqs = [letters[n] for n in names]
    assert [len(s) for s in seqs] == lens
    want = pl.model(records, names, lens, seqs, {"min_alt": 1, "min_pct": 0}, b"urmap -vcfout x")
    got = open(path("dev", "vcf"), "rb").read()
    assert got == want, first_difference(got, want)
    t = pl.parse(got)
    assert rep["pileup_sites"] == len(t["sites"]) >= 1 and rep["pileup_records"] > 100 and rep["pileup_s"] > 0
    assert rep["pileup_alt_alleles"] == sum(len(a) for _, _, _, a, _, _ in t["sites"]) and t["command"] == "urmap -vcfout x"
    for k, kw, env in (("host", {}, {"URMAPX_HOST_TEXT": "1"}), ("s2", {"streams": 2, "batch": 64}, {})):
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        api.map_files(index["index"], *fq, samout=path(k, "bam"), vcf_out=path(k, "vcf"), **common, **loose, **kw)
        assert open(path(k, "vcf"), "rb").read() == want, k
        for name in env:
            monkeypatch.delenv(name)
    # the defaults, beside the depth and the statistics; another MAPQ and quality floor
    api.map_files(index["index"], *fq, samout=path("def", "bam"), vcf_out=path("def", "vcf"), depth_out=path("def", "bed"), stats_out=path("def", "stats"), **common)
    assert open(path("def", "vcf"), "rb").read() == pl.model(records, names, lens, seqs, None, b"urmap -vcfout x")
    assert open(path("def", "bam"), "rb").read() == open(path("plain", "bam"), "rb").read()
    api.map_files(index["index"], *fq, samout=path("q", "bam"), vcf_out=path("q", "vcf"), vcf_mapq=30, vcf_baseq=25, vcf_min_alt=2, vcf_min_pct=1, **common)
    assert open(path("q", "vcf"), "rb").read() == pl.model(records, names, lens, seqs, {"min_mapq": 30, "min_baseq": 25, "min_alt": 2, "min_pct": 1}, b"urmap -vcfout x")
    # the refusals of the options
    for kw, word in ((dict(bam_sort=False, markdup=False), "vcf_out needs bam_sort"), (dict(vcf_out=""), "needs a file name"), (dict(vcf_out=path("no", "bam")), "file of their own"),
                     (dict(vcf_out=path("no", "bam") + ".bai"), "file of their own"), (dict(depth_out=path("no", "vcf")), "file of their own"),
                     (dict(stats_out=path("no", "vcf")), "file of their own"), (dict(vcf_min_alt=0), "vcf_min_alt"), (dict(vcf_min_pct=101), "vcf_min_pct"),
                     (dict(vcf_mapq=256), "vcf_mapq"), (dict(vcf_baseq=256), "vcf_baseq")):
        with pytest.raises(api.UrmapxError) as e:
            api.map_files(index["index"], *fq, samout=path("no", "bam"), **{**common, "vcf_out": path("no", "vcf"), **kw})
        assert e.value.code == api.E_ARG and word in str(e.value) and not os.path.exists(path("no", "bam")) and not os.path.exists(path("no", "vcf"))


def test_the_command_line(index):
    """urmap -map ... -bamout o.bam -sort -markdup -vcfout o.vcf: the file parses and is the model's for o.bam and g.fa; the @PG line
    names the flags; the same file with URMAPX_HOST_INDEX=1, where the bases are fetched and uploaded"""
    import subprocess
    exe = os.path.join(os.path.dirname(GOLD), "..", "urmap_amd", "urmap")
    out = {}
    for k, env in (("cli", {}), ("cli_host_index", {"URMAPX_HOST_INDEX": "1"})):
        bam, vcf = os.path.join(index["dir"], k + ".bam"), os.path.join(index["dir"], k + ".vcf")
        args = [exe, "-map", os.path.join(GOLD, "se150.fq"), "-ufi", index["ufi"], "-bamout", bam, "-sort", "-markdup", "-vcfout", vcf, "-vcf_min_alt", "1",
                "-vcf_min_pct", "0", "-vcf_baseq", "20"]
        r = subprocess.run(args, capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr
        out[k] = open(vcf, "rb").read()
    refs, records = records_of(bam)
    letters = fasta(os.path.join(GOLD, "g.fa"))
    names, lens = [n.decode() if isinstance(n, bytes) else n for n, _ in refs], [l for _, l in refs]
    t = pl.parse(out["cli"])
    assert "-vcfout" in t["command"] and "-vcf_baseq 20" in t["command"] and len(t["sites"]) >= 1
    assert out["cli"] == pl.model(records, names, lens, [letters[n] for n in names], {"min_baseq": 20, "min_alt": 1, "min_pct": 0}, t["command"].encode())
    assert out["cli_host_index"].split(b"\n")[3:] == out["cli"].split(b"\n")[3:]
    header = bl.read_bam(bl.inflate(open(bam, "rb").read()))[0]
    assert any(l.startswith(b"@PG") and b"-vcfout" in l and b"-vcf_min_pct 0" in l for l in header.split(b"\n"))


def test_map_files_with_an_index_that_is_not_resident(index):
    """an index with host arrays only: the bases are fetched once and uploaded; the same file"""
    from urmap_amd import api
    fq = os.path.join(GOLD, "se150.fq")
    path = lambda k, ext: os.path.join(index["dir"], "host_%s.%s" % (k, ext))  # noqa: E731
    common = dict(first_gpu=0, gpus=1, bam=True, bam_sort=True, markdup=True, cmdline="urmap -vcfout x", vcf_min_alt=1, vcf_min_pct=0)
    api.map_files(index["index"], fq, samout=path("res", "bam"), vcf_out=path("res", "vcf"), **common)
    api.map_files(api.Index.open(index["ufi"]), fq, samout=path("host", "bam"), vcf_out=path("host", "vcf"), **common)
    assert open(path("host", "vcf"), "rb").read() == open(path("res", "vcf"), "rb").read()
    assert len(pl.parse(open(path("host", "vcf"), "rb").read())["sites"]) >= 1
