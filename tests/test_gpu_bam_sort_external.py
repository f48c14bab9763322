"""GPU tests of the device sort's external road (urmapx_bam_sort_external; place_kernel in bam_sort.hip): the records stream through two
staging buffers while only the per-record arrays stay on the device.  Every case compares three results -- the external road, the host
function and the in-core device road -- as tests/test_gpu_bam_sort.py's `both` compares two: the inflated stream, the index in places of
the stream, the counters.  The partitions and the staged chunks are forced small with URMAPX_TEST_SORT_PARTITION / _STAGE, since the
compressor's fixed scratch dominates any budget at these sizes; one test plans from a budget alone."""
import contextlib
import os
import re

import numpy as np
import pytest

import bam_lib as bl
import bam_sort_lib as sl
import markdup_lib as ml
from test_bam_sort_cpu import check_sorted_file
from test_gpu_bam_sort import TINY, _run, both, golden, stable_order, tiny_records  # noqa: F401  (golden is a fixture)
from test_markdup_cpu import Q, R, pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
STATS = ("pairs_examined", "pairs_duplicate", "fragments_examined", "fragments_duplicate")
KNOBS = ("URMAPX_TEST_SORT_PARTITION", "URMAPX_TEST_SORT_STAGE")


@pytest.fixture(autouse=True)
def one_member_slices(monkeypatch):
    monkeypatch.setenv("URMAPX_TEST_SORT_SLICE", "1")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@contextlib.contextmanager
def slices_of_one_member():
    """for the module-scoped references, which are made before the function-scoped fixture above has run"""
    before = os.environ.get("URMAPX_TEST_SORT_SLICE")
    os.environ["URMAPX_TEST_SORT_SLICE"] = "1"
    try:
        yield
    finally:
        if before is None:
            del os.environ["URMAPX_TEST_SORT_SLICE"]
        else:
            os.environ["URMAPX_TEST_SORT_SLICE"] = before


def lengths(records):
    return [len(r) for _, r in sl.split_records(records)]


def chunk_starts(lens, stage, look=False):
    """the staged chunks of bam_sort.h's chunk_end: whole records of at most `stage` bytes, one at the least; under marking (look) the
    next chunk's first record is staged behind the chunk and counts"""
    offs = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
    n, cuts, i0 = len(lens), [], 0
    while i0 < n:
        cuts.append(i0)
        i1 = i0 + 1
        while i1 < n and offs[min(i1 + 1 + look, n)] - offs[i0] <= stage:
            i1 += 1
        i0 = i1
    return cuts


def external(monkeypatch, records, n_ref, partition, stage, in_front=0, markdup=False):
    """the external road with partitions of `partition` slices and staged chunks of `stage` bytes -> (stream, index in places, report,
    the file, the parsed index, the members' places)"""
    from urmap_amd import api
    monkeypatch.setenv(KNOBS[0], str(partition))
    monkeypatch.setenv(KNOBS[1], str(stage))
    try:
        em, ebai, erep = api.bam_sort(records, n_ref, device=0, bytes_in_front=in_front, report=True, markdup=markdup, budget=0)
    finally:
        for k in KNOBS:
            monkeypatch.delenv(k)
    return opened(em, ebai, erep, in_front)


def opened(em, ebai, erep, in_front=0):
    from urmap_amd import api
    f = sl.BgzfFile(b"\0" * in_front + em + api.BGZF_EOF)
    b, table = sl.parse_bai(ebai), sl.member_places(f, in_front)
    return bl.inflate(em), sl.index_in_places(b, table), erep, f, b, table


def agree(ext, ref):
    """ext: external()'s result, ref: `both`'s (the in-core device road, which `both` has held against the host)"""
    stream, b, f, table, rep = ref
    assert ext[0] == stream, "the external road's stream differs from the in-core road's and the host's"
    assert ext[1] == sl.index_in_places(b, table), "the external road's index differs"
    for k in ("stream_bytes", "records", "no_coor", "sort_passes", "slices"):
        assert ext[2][k] == rep[k], k
    assert ext[2]["external"] == 1 and rep["external"] == 0 and rep["partitions"] == 0


# ---- partitions x chunks ----
@pytest.fixture(scope="module")
def four_thousand():
    """the input of test_gpu_bam_sort.py::test_slices, and what the in-core road and the host make of it in slices of one member"""
    rng = np.random.default_rng(3)
    lines = [f"r{i}\t0\tc\t{int(rng.integers(1, 900000))}\t1\t{40 + i % 7}M\t*\t0\t0\t{'A' * (40 + i % 7)}\t{'#' * (40 + i % 7)}" for i in range(4000)]
    records = bl.sam_to_bam_records("\n".join(lines) + "\n", [("c", 1000000)])
    with slices_of_one_member():
        return records, both(records, 1)


@pytest.mark.parametrize("stage", [1, 4096, 1 << 30])
@pytest.mark.parametrize("partition", [1, 2, 3])
def test_partitions_and_chunks(monkeypatch, four_thousand, partition, stage):
    records, ref = four_thousand
    assert len(records) > 6 * sl.MEMBER
    ext = external(monkeypatch, records, 1, partition, stage)
    agree(ext, ref)
    rep = ext[2]
    assert rep["partitions"] == -(-len(records) // (partition * sl.MEMBER)) > 1
    want_chunks = len(chunk_starts(lengths(records), stage))
    assert rep["stage_chunks"] == want_chunks
    assert want_chunks == {1: 4000, 4096: want_chunks, 1 << 30: 1}[stage] and (stage != 4096 or 40 < want_chunks < 4000)
    cuts = [k * partition * sl.MEMBER for k in range(1, rep["partitions"])]
    recs = sl.split_records(ref[0])
    assert all(any(o < c < o + len(r) for o, r in recs) for c in cuts), "no record straddles a partition's end"


# ---- what the report says of each road ----
@pytest.mark.parametrize("markdup", [False, True])
def test_the_report_of_each_road(monkeypatch, four_thousand, markdup):
    """the counters and step times that only one road fills: slices of one member on both; gather_s in core, where nothing is staged;
    partitions, staged chunks (bam_sort.h's chunk_end over the records' lengths) and stage_s on the external road, where nothing is
    gathered; the same coordinate sort on both; under marking its time on both"""
    from urmap_amd import api
    records, _ = four_thousand
    slices = -(-len(records) // sl.MEMBER)
    core = api.bam_sort(records, 1, device=0, report=True, markdup=markdup)[2]
    assert core["slices"] == slices and core["partitions"] == 0 and core["stage_chunks"] == 0
    assert core["stage_s"] == 0 and core["gather_s"] > 0
    ext = external(monkeypatch, records, 1, 2, 4096, markdup=markdup)[2]
    assert ext["slices"] == slices and ext["partitions"] == -(-slices // 2)
    assert ext["stage_chunks"] == len(chunk_starts(lengths(records), 4096, look=markdup))
    assert ext["gather_s"] == 0 and ext["stage_s"] > 0
    assert ext["sort_passes"] == core["sort_passes"] > 0
    if markdup:
        assert core["markdup_s"] > 0 and ext["markdup_s"] > 0


# ---- a record longer than a partition ----
@pytest.mark.parametrize("pushed", [False, True])
def test_a_record_longer_than_a_partition(monkeypatch, pushed):
    """the input of test_gather_shapes: a 70 000-base record (the staging buffers must grow to it), names of every length mod 4, a
    41-op CIGAR, bytes in front of the first member.  That record is 105 045 bytes and lies at 8 913 of the sorted stream, so with
    partitions of one member it begins in the first and ends in the second; `pushed`: the same input with 500 records more in front
    of it, so that it begins in the first partition, covers the second whole and ends in the third"""
    refs = [("a", 300000), ("b", 300000)]
    rng = np.random.default_rng(11)
    lines = []
    for i in range(400):
        name = "n" * (1 + i % 9)
        p = int(rng.integers(1, 200000))
        if i % 50 == 7:
            cigar, q = "".join("3M1I" if k % 2 else "3M1D" for k in range(20)) + "5M", 3 * 20 + 10 + 5
        else:
            cigar, q = "%dM" % (30 + i % 5), 30 + i % 5
        lines.append(f"{name}\t0\t{refs[i % 2][0]}\t{p}\t9\t{cigar}\t*\t0\t0\t{'ACGT'[i % 4] * q}\t{'F' * q}")
    lines.insert(123, "long\t0\ta\t100000\t9\t70000M\t*\t0\t0\t%s\t%s" % ("C" * 70000, "G" * 70000))
    lines.insert(300, "u\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*")
    records = bl.sam_to_bam_records("\n".join(lines) + "\n", refs) + tiny_records([0, -1, 1], [5, -1, 299999])
    if pushed:
        records += tiny_records(np.zeros(500, int), np.arange(500))
    assert max(lengths(records)) > sl.MEMBER + 36
    ext = external(monkeypatch, records, 2, 1, 4096, in_front=1234)
    agree(ext, both(records, 2, in_front=1234))
    stream, _, rep, f, b, table = ext
    assert rep["partitions"] == -(-len(records) // sl.MEMBER)
    at, long_rec = max(sl.split_records(stream), key=lambda x: len(x[1]))
    assert (at // sl.MEMBER, (at + len(long_rec) - 1) // sl.MEMBER) == ((0, 2) if pushed else (0, 1)), "the long record does not lie across the partitions' ends"
    _, recs = sl.check_stream(f.blob[1234:-28], records)
    assert set(o % 4 for o, _ in recs) == {0, 1, 2, 3}
    sl.check_index(b, recs, table, 2)
    sl.check_queries(b, f, [r for _, r in recs], [(0, 0, 10), (0, 99999, 100000), (0, 169998, 169999), (0, 169999, 170001), (1, 299999, 300000), (1, 0, 300000)])


# ---- edges ----
@pytest.mark.parametrize("n", [0, 1])
def test_no_record_and_one(monkeypatch, n):
    records = tiny_records(np.zeros(n, int), np.full(n, 7))
    ext = external(monkeypatch, records, 1, 1, 1)
    agree(ext, both(records, 1))
    assert ext[2]["partitions"] == n and ext[2]["stage_chunks"] == n


def test_the_last_partition_ends_at_the_streams_end(monkeypatch):
    """3264 records of 40 bytes are exactly two members: two partitions, not three"""
    n = 3264
    a = np.frombuffer(tiny_records(np.zeros(n, int), (np.arange(n) * 7919) % 100000), TINY)
    wide = np.dtype(TINY.descr[:-1] + [("name", "S4")])
    w = np.zeros(n, wide)
    for k in TINY.names:
        w[k] = a[k]
    w["block_size"], w["l_name"], w["name"] = 36, 4, b"abc"
    records = w.tobytes()
    assert len(records) == 2 * sl.MEMBER
    ext = external(monkeypatch, records, 1, 1, 4096)
    agree(ext, both(records, 1))
    assert ext[2]["partitions"] == 2 and ext[2]["slices"] == 2
    assert (np.frombuffer(ext[0], wide)["tlen"] == stable_order(np.zeros(n, int), w["pos"])).all()


def test_all_records_unplaced(monkeypatch):
    n = 2500
    records = tiny_records(np.full(n, -1), np.full(n, -1))
    ext = external(monkeypatch, records, 3, 1, 4096)
    agree(ext, both(records, 3))
    assert ext[2]["no_coor"] == n and ext[2]["partitions"] == 2
    assert (np.frombuffer(ext[0], TINY)["tlen"] == np.arange(n)).all()


def test_one_key_keeps_the_input_order_a_record_a_chunk(monkeypatch):
    n = 1000
    records = tiny_records(np.zeros(n, int), np.full(n, 777))
    ext = external(monkeypatch, records, 1, 1, 1)
    agree(ext, both(records, 1))
    assert ext[2]["partitions"] == 1 and ext[2]["stage_chunks"] == n  # (38 000 bytes: one member)
    big = records + tiny_records(np.zeros(n, int), np.full(n, 777))  # two members: the same across two partitions
    ext = external(monkeypatch, big, 1, 1, 1)
    agree(ext, both(big, 1))
    assert ext[2]["partitions"] == 2 and ext[2]["stage_chunks"] == 2 * n
    assert (np.frombuffer(ext[0], TINY)["tlen"] == np.concatenate([np.arange(n), np.arange(n)])).all()


# ---- keys across chunks ----
def test_keys_across_chunks_beyond_one_tile_a_workgroup(monkeypatch):
    n = 512 * 1024 + 1
    rng = np.random.default_rng(n)
    n_ref = 300
    ref = rng.integers(-1, n_ref, n)
    pos = np.where(ref < 0, -1, rng.integers(0, 1 << 20, n))
    records = tiny_records(ref, pos)
    ext = external(monkeypatch, records, n_ref, 64, 1 << 20)
    agree(ext, both(records, n_ref))
    assert (np.frombuffer(ext[0], TINY)["tlen"] == stable_order(ref, pos)).all()
    assert ext[2]["sort_passes"] == 4
    assert ext[2]["partitions"] == -(-len(records) // (64 * sl.MEMBER)) and ext[2]["stage_chunks"] == -(-n // ((1 << 20) // 38))


# ---- markdup ----
def marked_input():
    """pairs (FR and RF, duplicates of each other), fragments on pair ends and elsewhere, ties in the score, ineligible records and
    incoming 0x400 bits; names of several lengths so that records start at every address residue"""
    rng = np.random.default_rng(4)
    recs = []
    for i in range(1000):
        q = lambda: bytes(rng.integers(10, 41, 20, dtype=np.uint8))  # noqa: E731
        a, b = (0, 100 * int(rng.integers(0, 6)), 0), (0, 5000 + 100 * int(rng.integers(0, 6)), 1)
        name = b"p%d" % i + b"x" * (i % 4)
        if i % 2:
            recs += pair(name, *((a, b) if i % 3 else (b, a)), qa=q() if i % 5 else Q(30), qb=q() if i % 5 else Q(30))
        elif i % 7 == 0:
            recs += [R(1, 40 * i, 0x4 if i % 14 else 0x900, "20M", q(), name), R(2, 100, 0x400, "20M", Q(30), name)]
        else:
            recs += [R(*a[:2], 0, "20M", q() if i % 3 else Q(30), name), R(*b[:2], 16, "20M", q(), name + b"g")]
    return recs


@pytest.fixture(scope="module")
def marked():
    from urmap_amd import api
    recs = marked_input()
    raw = b"".join(recs)
    with slices_of_one_member():
        dm, dbai, drep = api.bam_sort(raw, 3, device=0, report=True, markdup=True)
        hm, hbai, hrep = api.bam_sort_host(raw, 3, report=True, markdup=True)
    d, h = opened(dm, dbai, drep), opened(hm, hbai, hrep)
    assert d[0] == h[0] and d[1] == h[1]
    assert len(raw) > 2 * sl.MEMBER and hrep["pairs_duplicate"] > 50 and hrep["fragments_duplicate"] > 50
    return recs, raw, d, h


def stages_for_marked():
    """one record a chunk (every pair straddles a chunk's end), and the two sizes that put a chunk's end just in front of and just
    behind the first mate of one pair"""
    recs = marked_input()
    lens = [len(r) for r in recs]
    offs = np.concatenate([[0], np.cumsum(lens)])
    j = next(i for i in range(200, len(recs) - 1) if ml.core(recs[i])[4] & 0x41 == 0x41 and ml.core(recs[i + 1])[4] & 0x81 == 0x81)
    return j, [1, int(offs[j + 1]), int(offs[j + 2])]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_markdup(monkeypatch, marked, which):
    recs, raw, d, h = marked
    j, stages = stages_for_marked()
    stage = stages[which]
    cuts = chunk_starts([len(r) for r in recs], stage, look=True)
    if which == 1:
        assert cuts[1] == j  # the first chunk ends in front of the pair's first mate
    if which == 2:
        assert cuts[1] == j + 1  # ... and here between the mates
    ext = external(monkeypatch, raw, 3, 1, stage, markdup=True)
    assert ext[2]["stage_chunks"] == len(cuts) and ext[2]["partitions"] == -(-len(raw) // sl.MEMBER) > 2
    for other in (d, h):
        assert ext[0] == other[0] and ext[1] == other[1]
        for k in ("stream_bytes", "records", "no_coor") + STATS:
            assert ext[2][k] == other[2][k], k
    plain = external(monkeypatch, raw, 3, 1, stage)
    assert ml.mask_dup(ext[0]) == ml.mask_dup(plain[0]) and ext[1] == plain[1]
    ml.check(raw, ext[0], plain[0], ext[2])


# ---- a budget and no knob ----
def test_a_budget_alone_chooses_the_road(monkeypatch):
    from urmap_amd import api
    import ctypes as C
    n = 20000
    rng = np.random.default_rng(8)
    recs = [R(int(rng.integers(0, 3)), int(rng.integers(0, 1 << 20)), 0, "30M", Q(30, 30), b"read%05d" % i) for i in range(n)]
    raw = b"".join(recs)
    assert 90 <= len(raw) / n <= 110
    L = api.lib()
    L.urmapx_bam_sort_device_bytes.restype, L.urmapx_bam_sort_device_bytes.argtypes = C.c_uint64, [C.c_size_t, C.c_uint64]
    need = int(L.urmapx_bam_sort_device_bytes(len(raw), n))
    ref = both(raw, 3)
    budget = need - 4 * 65536
    em, ebai, erep = api.bam_sort(raw, 3, device=0, report=True, budget=budget)
    plan = api.bam_sort_plan(len(raw), n, budget)
    assert erep["external"] == 1 and erep["partitions"] == plan["partitions"] >= 2
    agree(opened(em, ebai, erep), ref)
    im, ibai, irep = api.bam_sort(raw, 3, device=0, report=True, budget=need)
    assert irep["external"] == 0 and irep["partitions"] == 0 and irep["stage_chunks"] == 0
    assert bl.inflate(im) == ref[0]


# ---- the command line ----
INPUTS = {"se": (["-map", os.path.join(GOLD, "se150.fq")], "g"),
          "pe": (["-map2", os.path.join(GOLD, "pe120_rep_1.fq"), "-reverse", os.path.join(GOLD, "pe120_rep_2.fq")], "r")}
MARK_LINE = rb"Seconds to mark duplicates: (\d+) of (\d+) pairs, (\d+) of (\d+) fragments"


def records_of(path):
    """the inflated record stream of a BAM file and its index in places of that stream"""
    blob = open(path, "rb").read()
    data = bl.inflate(blob)
    l_text, = np.frombuffer(data, "<u4", 1, 4)
    at = 8 + int(l_text)
    n_ref, = np.frombuffer(data, "<u4", 1, at)
    at += 4
    for _ in range(int(n_ref)):
        l_name, = np.frombuffer(data, "<u4", 1, at)
        at += 8 + int(l_name)
    f = sl.BgzfFile(blob)
    in_front = f.member(0)[1]
    return data[at:], sl.index_in_places(sl.parse_bai(open(path + ".bai", "rb").read()), sl.member_places(f, in_front))


@pytest.mark.parametrize("markdup", [False, True])
@pytest.mark.parametrize("kind", ["se", "pe"])
def test_cli(golden, kind, markdup):  # noqa: F811
    args = INPUTS[kind][0] + ["-ufi", golden[INPUTS[kind][1]]]
    tail = ["-sort"] + (["-markdup"] if markdup else []) + ["-tags", "NM,MD,AS"]
    paths = {k: os.path.join(golden["dir"], f"ext_{kind}_{int(markdup)}_{k}.bam") for k in ("unsorted", "core", "ext", "mem")}
    env = {**os.environ, "URMAPX_VERBOSE": "1"}
    core = _run(args + ["-bamout", paths["core"]] + tail, env=env)
    ext = _run(args + ["-bamout", paths["ext"]] + tail, env={**env, "URMAPX_TEST_SORT_PARTITION": "1", "URMAPX_TEST_SORT_STAGE": "4096"})
    want, got = records_of(paths["core"]), records_of(paths["ext"])
    assert got[0] == want[0] and got[1] == want[1]
    m = re.search(rb"bam_sort external: partitions (\d+) chunks (\d+)", ext.stderr)
    assert m and int(m.group(1)) == -(-len(got[0]) // sl.MEMBER) >= 2 and int(m.group(2)) > 10, ext.stderr
    assert b"bam_sort external" not in core.stderr and b"bam_sort seconds:" in ext.stderr
    if markdup:
        assert re.search(MARK_LINE, ext.stderr).groups() == re.search(MARK_LINE, core.stderr).groups()
    else:  # (the yardstick's reader of whole files takes no optional fields: the same run without them)
        plain = [a for a in tail if a not in ("-tags", "NM,MD,AS")]
        _run(args + ["-quiet", "-bamout", paths["unsorted"]])
        _run(args + ["-quiet", "-bamout", paths["ext"]] + plain, env={**env, "URMAPX_TEST_SORT_PARTITION": "1", "URMAPX_TEST_SORT_STAGE": "4096"})
        check_sorted_file(open(paths["ext"], "rb").read(), open(paths["ext"] + ".bai", "rb").read(), open(paths["unsorted"], "rb").read())
    # -sortmem 64G: everything fits, the in-core run (the @PG line holds the command line, so the header differs; the records do not)
    mem = _run(args + ["-bamout", paths["mem"]] + tail + ["-sortmem", "64G"], env=env)
    assert b"bam_sort external" not in mem.stderr and records_of(paths["mem"]) == want


def test_cli_refusals(golden):  # noqa: F811
    args = INPUTS["se"][0] + ["-ufi", golden["g"], "-quiet"]
    out = os.path.join(golden["dir"], "ext_no.bam")
    r = _run(args + ["-bamout", out, "-sort", "-sortmem", "1"], ok=False)
    m = re.search(rb"at least (\d+) bytes", r.stderr)
    assert r.returncode != 0 and m and int(m.group(1)) > 1 << 20 and b"sort_mem" in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".bai")
    none = ["-map", os.path.join(GOLD, "se150.fq"), "-ufi", os.path.join(golden["dir"], "no_such.ufi"), "-quiet"]  # (refused before the index is opened)
    for extra, word in ((["-bamout", out, "-sortmem", "1G"], b"-sort"), (["-bamout", out, "-sort", "-sortmem", "12x"], b"12x"),
                        (["-bamout", out, "-sort", "-sortmem", "0"], b"-sortmem")):
        r = _run(none + extra, ok=False)
        assert r.returncode != 0 and b"-sortmem" in r.stderr and word in r.stderr and b"no_such" not in r.stderr and len(r.stderr.strip().split(b"\n")) == 2, r.stderr
        assert r.stdout == b"" and not os.path.exists(out) and not os.path.exists(out + ".bai")
