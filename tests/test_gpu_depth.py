"""GPU: per-base depth on the device (urmapx_bam_depth, urmapx_bam_sort_with; depth.hip) against the host version (depth_host.cpp) and the
model of tests/depth_lib.py: text bytes, run count and summaries, at the edges of the kernels' grids, tiles, segments and slices."""
import ctypes as C
import os

import numpy as np
import pytest

import bam_lib as bl
import depth_lib as dl
import markdup_lib as ml
from test_depth_cpu import agree, duplicated_input
from test_markdup_cpu import Q, pair

pytestmark = pytest.mark.gpu

# depth.h
NT = 256                    # records a workgroup of depth_count_kernel takes at a time
COUNT_BLOCKS = 1024         # its workgroups at the most: beyond COUNT_BLOCKS * NT records in a chunk a thread takes several
LANE_OPS = 8                # CIGAR ops a lane walks alone
SCAN_TILE = 2048            # counters a workgroup scans at a time
SCAN_BLOCKS = 1024          # workgroups of the scan: beyond SCAN_BLOCKS * SCAN_TILE counters each takes several tiles
SEGMENT = 2048 * 1024       # counters whose run starts are found at a time
TEXT_RUNS = 65536           # lines of a slice of the text
KNOBS = ("URMAPX_TEST_SORT_STAGE", "URMAPX_TEST_SORT_PARTITION", "URMAPX_TEST_SORT_SLICE", "URMAPX_TEST_DEPTH_SLICE")
R = dl.R


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def spans(ref_ids, positions, lengths):
    """many records of dl.span's shape at once: one template, its refID, pos and op length patched (the bin is left alone: no depth reads it)"""
    n = len(positions)
    t = np.frombuffer(dl.span(0, 0, 1), dtype=np.uint8)
    out = np.tile(t, (n, 1))
    out[:, 4:8] = np.asarray(ref_ids, dtype="<i4").reshape(n, 1).view(np.uint8)
    out[:, 8:12] = np.asarray(positions, dtype="<i4").reshape(n, 1).view(np.uint8)
    out[:, len(t) - 4:] = (np.asarray(lengths, dtype="<u4") << 4).reshape(n, 1).view(np.uint8)
    return out.tobytes()


def device_host_model(records, names, lens, min_mapq=0, model=True):
    """the device result, held against the host's and (model) the model's -> (text, runs, summaries, report)"""
    from urmap_amd import api
    got = api.bam_depth(records, len(lens), names, lens, device=0, min_mapq=min_mapq, report=True)
    agree(got, api.bam_depth_host(records, len(lens), names, lens, min_mapq=min_mapq))
    if model:
        agree(got, dl.model(records, names, lens, min_mapq))
    return got


# ---- grid edges of the counting kernel ----
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, NT + 1, 4 * NT + 1, COUNT_BLOCKS * NT + 1])
def test_record_counts(monkeypatch, n):
    rng = np.random.default_rng(n)
    lens = [5000, 1, 3000]
    refs = rng.integers(0, 3, n)
    pos = rng.integers(0, 5100, n) % (np.asarray(lens)[refs] + 40)  # (some begin beyond their reference's end)
    records = spans(refs, pos, rng.integers(1, 200, n))
    assert len(records) == 42 * n
    monkeypatch.setenv("URMAPX_TEST_SORT_STAGE", str(1 << 30))  # one chunk: every record in one launch
    text, runs, summ, rep = device_host_model(records, ["a", "b", "c"], lens, model=n <= 4 * NT + 1)
    assert rep["records"] == n and rep["stage_chunks"] == (1 if n else 0) and sum(s["reads"] for s in summ) == n
    if n > 4 * NT + 1:  # too many for the model: a prefix as an input of its own
        device_host_model(records[:42 * 3000], ["a", "b", "c"], lens)


# ---- tiles and rounds of the scan, segments of the run search ----
def edge_records(lens, rng, n=1500):
    """spans that crowd the ends of every reference, some hanging over them"""
    first = np.concatenate([[0], np.cumsum(lens)])
    refs = rng.integers(0, len(lens), n)
    l = np.asarray(lens)[refs]
    near_end = rng.random(n) < 0.5
    pos = np.where(near_end, np.maximum(l - rng.integers(0, 40, n), 0), rng.integers(0, 1 << 30, n) % np.maximum(l, 1))
    keep = l > 0
    return spans(refs[keep], pos[keep], rng.integers(1, 60, n)[keep]), first


@pytest.mark.parametrize("entries", [SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, SCAN_BLOCKS * SCAN_TILE + 1, SEGMENT + SCAN_TILE + 3])
def test_counter_counts(entries):
    """one reference whose counters (its columns and the one entry more) are `entries`: a tile less one, a tile, a tile and one, one more
    than the scan's grid covers at a tile a workgroup (every workgroup then walks two), and a second segment of the run search"""
    lens = [entries - 1]
    rng = np.random.default_rng(entries)
    records, _ = edge_records(lens, rng)
    records += dl.span(0, entries - 2, 1) + dl.span(0, 0, 1) + dl.span(0, SCAN_TILE - 3, 9)  # the last column, the first, across a tile's end
    if entries > SEGMENT:
        records += dl.span(0, SEGMENT - 5, 10) + dl.span(0, SEGMENT, 1) * 3 + dl.span(0, SEGMENT - 1, 1)  # runs that end and begin on the segment's edge
    text, runs, summ, rep = device_host_model(records, ["chr"], lens)
    dl.check_tiling(text, ["chr"], lens)
    assert summ[0]["covered"] > 0


@pytest.mark.parametrize("shift", [-1, 0, 1])
@pytest.mark.parametrize("where", [SCAN_TILE, 2 * SCAN_TILE * 3, SEGMENT])
def test_a_reference_boundary_at_a_tile_boundary(where, shift):
    """the first reference's counters end at a tile's, at a workgroup's range's (two tiles each at this size) or at the segment's end, and
    one column to either side"""
    total = SCAN_BLOCKS * SCAN_TILE + 1 if where < SEGMENT else SEGMENT + 3 * SCAN_TILE
    first = where + shift          # counters of the first reference
    lens = [first - 1, 0, 1, total - first - 3 - 1]
    assert sum(lens) + len(lens) == total
    rng = np.random.default_rng(where + shift)
    records, _ = edge_records(lens, rng)
    records += dl.span(0, lens[0] - 1, 5) + dl.span(2, 0, 2) + dl.span(3, 0, 1) + dl.span(3, lens[3] - 1, 1)
    names = ["one", "none", "x", "two"]
    text, runs, summ, rep = device_host_model(records, names, lens)
    dl.check_tiling(text, names, lens)


# ---- many atomics on two addresses ----
def test_contention():
    records, names, lens = dl.digits_case(100000)
    text, runs, summ, rep = device_host_model(records, names, lens)
    assert text == b"d\t0\t5\t0\nd\t5\t25\t100000\nd\t25\t30\t0\n" and summ == [dict(reads=100000, covered=20, bases=2000000, mapq_sum=0)]


# ---- runs at their extremes ----
def test_a_staircase_in_several_text_slices(monkeypatch):
    n = 5000
    lens, names = [7, n, 3], ["lo", "stairs", "hi"]
    records = spans(np.ones(n, dtype=int), np.arange(n), n - np.arange(n))  # column x is covered by x + 1 records
    monkeypatch.setenv("URMAPX_TEST_DEPTH_SLICE", "700")
    text, runs, summ, rep = device_host_model(records, names, lens)
    assert runs == n + 2 and rep["text_slices"] == -(-runs // 700)
    assert dl.parse(text)[1:3] == [(b"stairs", 0, 1, 1), (b"stairs", 1, 2, 2)] and summ[1]["bases"] == n * (n + 1) // 2
    monkeypatch.setenv("URMAPX_TEST_DEPTH_SLICE", "1")
    few = spans(np.ones(40, dtype=int), np.arange(40), 40 - np.arange(40))
    assert device_host_model(few, names, [7, 40, 3])[3]["text_slices"] == 42


def test_an_empty_genome():
    rng = np.random.default_rng(5)
    lens = [int(x) for x in rng.integers(0, 4000, 300)]
    lens[7] = lens[8] = 0
    names = ["contig_%d" % k for k in range(300)]
    text, runs, summ, rep = device_host_model(b"", names, lens)
    assert runs == sum(1 for l in lens if l) and rep["text_slices"] == 1
    assert dl.parse(text) == [(n.encode(), 0, l, 0) for n, l in zip(names, lens) if l]


# ---- CIGAR shapes ----
def long_cigar(n_ops):
    unit = ["3M", "1I", "2D", "4=", "1S", "5N", "2X", "1P", "1H", "1M"]
    return "".join(unit[k % len(unit)] for k in range(n_ops))


@pytest.mark.parametrize("min_mapq", [0, 17, 18])
def test_cigar_cases(min_mapq):
    records, names, lens = dl.cigar_cases()
    device_host_model(records, names, lens, min_mapq)


def test_long_cigars_are_shared_by_the_wavefront():
    """1 000 and 65 535 ops, the latter hanging over its reference's end; CIGARs of LANE_OPS and LANE_OPS + 1 ops; short ones in the same
    wavefront before, between and behind them"""
    names, lens = ["a", "b"], [3000, 100000]
    recs = [R(0, 5 + k, 0, "7M", b"") for k in range(20)]
    recs += [R(0, 10, 0, long_cigar(1000), b""), R(1, 3, 0, long_cigar(LANE_OPS), b""), R(1, 4, 0, long_cigar(LANE_OPS + 1), b"")]
    recs += [R(1, 50 + k, 0, "2M3D2M", b"") for k in range(30)]
    recs += [R(1, 7, 0, long_cigar(65535), b""), R(1, 9, 0x400, long_cigar(70), b""), R(1, 11, 0, long_cigar(64), b""), R(1, 12, 0, long_cigar(65), b"")]
    recs += [R(0, 2990, 0, "20M", b"")]
    text, runs, summ, rep = device_host_model(b"".join(recs), names, lens)
    assert summ[1]["reads"] == 35 and runs > 10000


# ---- staging ----
@pytest.mark.parametrize("stage", [1, 300])
def test_staged_chunks(monkeypatch, stage):
    records, names, lens = dl.cigar_cases()
    records += R(0, 3, 0, long_cigar(200), b"") + dl.span(4, 1, 30) * 5
    n = len(ml.flags_of(records))
    monkeypatch.setenv("URMAPX_TEST_SORT_STAGE", str(stage))
    text, runs, summ, rep = device_host_model(records, names, lens)
    assert rep["stage_chunks"] == n if stage == 1 else 3 < rep["stage_chunks"] < n


# ---- with the sort ----
def many_duplicates():
    """3 000 records in 1 500 pairs at 500 places -- two of every three pairs are duplicates -- and lone reads between them, in no order"""
    rng = np.random.default_rng(11)
    recs = []
    for k in rng.permutation(1500):
        at = 200 + 31 * int(k % 500)
        recs += pair(b"p%04d" % k, (int(k % 2), at, 0), (int(k % 2), at + 170, 1), qa=Q(20 + int(k % 17)), qb=Q(30))
        if k % 5 == 0:
            recs.append(R(2, int(k), 0x400 if k % 10 else 0, "15M", Q(30), b"lone%d" % k))
    return b"".join(recs), ["r0", "r1", "r2"], [20000, 16000, 1400]


@pytest.mark.parametrize("road", ["in core", "external"])
def test_with_the_sort_the_flags_are_those_written_and_every_record_counts_once(monkeypatch, road):
    from urmap_amd import api
    records, names, lens = many_duplicates()
    if road == "external":
        monkeypatch.setenv("URMAPX_TEST_SORT_SLICE", "1")
        monkeypatch.setenv("URMAPX_TEST_SORT_PARTITION", "1")
        monkeypatch.setenv("URMAPX_TEST_SORT_STAGE", "5000")
    members, bai, depth, rep = api.bam_sort(records, 3, markdup=True, budget=0, depth=(names, lens), report=True)
    assert (members, bai) == api.bam_sort(records, 3, markdup=True, budget=0)[:2], "the depth changed the file or its index"
    assert (rep["external"], rep["partitions"] >= 3) == ((1, True) if road == "external" else (0, False))
    stream = bl.inflate(members)
    flags = ml.flags_of(stream)
    assert sum(1 for f in flags if f & 0x400) * 4 >= len(flags) and rep["pairs_duplicate"] == 1000
    agree(depth, api.bam_depth_host(stream, 3, names, lens))
    agree(depth, dl.model(stream, names, lens))
    assert depth[2] != dl.model(records, names, lens)[2]  # (the incoming flags give another answer)
    assert rep["depth_records"] == len(flags)
    # without marking, and with a least MAPQ no record has: the flags as they came; nothing
    _, _, plain = api.bam_sort(records, 3, budget=0, depth=(names, lens))
    agree(plain, dl.model(records, names, lens))
    _, _, none = api.bam_sort(records, 3, markdup=True, budget=0, depth=(names, lens), depth_mapq=1)
    agree(none, dl.model(b"", names, lens))


def test_the_small_inputs_of_the_cpu_tests_through_the_sort(monkeypatch):
    from urmap_amd import api
    records, names, lens = duplicated_input()
    for knobs in ({}, {"URMAPX_TEST_SORT_SLICE": "1", "URMAPX_TEST_SORT_PARTITION": "1", "URMAPX_TEST_SORT_STAGE": "1"}):
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        members, bai, depth = api.bam_sort(records, 3, markdup=True, budget=0, depth=(names, lens))
        agree(depth, api.bam_sort_host(records, 3, markdup=True, depth=(names, lens))[2])
        agree(depth, dl.model(bl.inflate(members), names, lens))
    members, bai, depth = api.bam_sort(b"", 3, markdup=True, budget=0, depth=(names, lens))
    agree(depth, dl.model(b"", names, lens))


def test_a_budget_that_does_not_hold_the_counters_names_the_least():
    from urmap_amd import api
    records, names, lens = duplicated_input()
    lens = [1000, 800, 40 << 20]  # 160 MiB of counters
    own = api.bam_depth_resident_bytes(sum(lens), 3)
    assert own > 4 * sum(lens)
    for budget in (1000, own, own + (1 << 20)):
        with pytest.raises(api.UrmapxError) as e:
            api.bam_sort(records, 3, markdup=True, budget=budget, depth=(names, lens))
        assert e.value.code == -3 and e.value.least_budget > own and str(e.value.least_budget) in str(e.value)
    # the least budget holds the call (a staged chunk that had to grow for a long record raises it once more, and says so)
    least = e.value.least_budget
    for _ in range(3):
        try:
            members, bai, depth = api.bam_sort(records, 3, markdup=True, budget=least, depth=(names, lens))
            break
        except api.UrmapxError as again:
            assert again.code == -3 and again.least_budget > least
            least = again.least_budget
    with pytest.raises(api.UrmapxError):
        api.bam_sort(records, 3, markdup=True, budget=least - 1, depth=(names, lens))
    agree(depth, api.bam_sort_host(records, 3, markdup=True, depth=(names, lens))[2])


# ---- the command line ----
from test_depth_cpu import records_and_refs  # noqa: E402
from test_gpu_bam_sort import _run, golden  # noqa: E402,F401  (golden is a fixture)
from test_gpu_bam_sort_external import records_of  # noqa: E402
from test_gpu_multi import _force_env  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("reads,ufi", [("pe150", "g"), ("pe120_rep", "r")])
def test_cli(monkeypatch, golden, reads, ufi):  # noqa: F811
    """-sort -markdup -depth on the golden pairs: the file is the model's for the records the BAM file holds; the same file under -host,
    on two devices and streamed; the BAM file's records and index are those of the run without -depth"""
    args = ["-map2", os.path.join(GOLD, reads + "_1.fq"), "-reverse", os.path.join(GOLD, reads + "_2.fq"), "-ufi", golden[ufi]]
    path = lambda k, ext: os.path.join(golden["dir"], f"depth_{reads}_{k}.{ext}")  # noqa: E731
    _run(args + ["-quiet", "-bamout", path("plain", "bam"), "-sort", "-markdup"])
    env = {**os.environ, "URMAPX_VERBOSE": "1"}
    r = _run(args + ["-bamout", path("dev", "bam"), "-sort", "-markdup", "-depth", path("dev", "bedgraph")], env=env)
    assert records_of(path("dev", "bam")) == records_of(path("plain", "bam"))
    header = bl.read_bam(bl.inflate(open(path("dev", "bam"), "rb").read()))[0]
    assert b"-depth " in [l for l in header.split(b"\n") if l.startswith(b"@PG")][0]
    records, names, lens = records_and_refs(path("dev", "bam"))
    want, runs, summ = dl.model(records, names, lens)
    got = open(path("dev", "bedgraph"), "rb").read()
    assert got == want and sum(s["reads"] for s in summ) > 100
    dl.check_tiling(got, names, lens)
    assert b"depth seconds: total" in r.stderr and b"runs %d bytes %d" % (runs, len(want)) in r.stderr
    for name, l, s in zip(names, lens, summ):  # the table per reference
        assert ("%s\t%d\t%d\t%d\t%.2f\t" % (name, l, s["reads"], s["covered"], 100.0 * s["covered"] / l)).encode() in r.stderr, r.stderr
    # the other roads write the same file.  -sortmem: one byte less than the depth arrays and the in-core sort take, so the records stream
    from urmap_amd import api
    monkeypatch.setenv("URMAPX_TEST_SORT_SLICE", "1")
    in_core = api.lib().urmapx_bam_sort_markdup_device_bytes
    in_core.restype, in_core.argtypes = C.c_uint64, [C.c_size_t, C.c_uint64]
    sort_mem = api.bam_depth_resident_bytes(sum(lens), len(lens)) + int(in_core(len(records), len(ml.flags_of(records)))) - 1
    for k, extra, e in (("host", ["-host"], env), ("two", ["-gpus", "2", "-streams", "2", "-batch", "60"], {**_force_env(), "URMAPX_VERBOSE": "1"}),
                        ("mem", ["-sortmem", str(sort_mem)], {**env, "URMAPX_TEST_SORT_SLICE": "1"})):
        r = _run(args + ["-quiet", "-bamout", path(k, "bam"), "-sort", "-markdup", "-depth", path(k, "bedgraph")] + extra, env=e)
        assert open(path(k, "bedgraph"), "rb").read() == want, k
        assert records_of(path(k, "bam"))[0] == records
        if k == "mem":
            assert b"bam_sort external: partitions" in r.stderr, r.stderr
    # a least MAPQ
    _run(args + ["-quiet", "-bamout", path("q", "bam"), "-sort", "-markdup", "-depth", path("q", "bedgraph"), "-depth_mapq", "20"])
    assert open(path("q", "bedgraph"), "rb").read() == dl.model(records, names, lens, 20)[0] != want


def test_cli_a_budget_too_small_for_the_counters(golden):  # noqa: F811
    args = ["-map", os.path.join(GOLD, "se150.fq"), "-ufi", golden["g"], "-quiet"]
    out, bed = os.path.join(golden["dir"], "depth_no.bam"), os.path.join(golden["dir"], "depth_no.bedgraph")
    r = _run(args + ["-bamout", out, "-sort", "-depth", bed, "-sortmem", "100K"], ok=False)
    assert r.returncode != 0 and b"at least" in r.stderr and b"sort_mem" in r.stderr and b"depth" in r.stderr, r.stderr
    assert int(r.stderr.split(b"at least ")[1].split()[0]) > 100 << 10
    assert not os.path.exists(out) and not os.path.exists(out + ".bai") and not os.path.exists(bed)
