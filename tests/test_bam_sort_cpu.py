"""Sorted BAM output, host side: urmapx_bam_sort_host on synthetic records against the yardstick of tests/bam_sort_lib.py -- order,
cuts, every property of the index, region queries through the index against brute force --, its refusals, and urmapx_map_files with
bam_sort set through the sanitizer builds' stand-alone programs (the device stand-in sorts with the host function)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bam_lib as bl
import bam_sort_lib as sl
from urmap_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SAN_DIR = os.path.join(ROOT, "urmap_amd", "csrc", "build_san")

REFS = [("big", (1 << 26) + 90000), ("mid", 40000), ("none", 5000), ("small", 20000)]  # "none" gets no record


def synthetic_sam(seed=1, n=1500):
    """SAM lines whose positions crowd the places where an index goes wrong: position 0, a reference's last base, both sides of 2^14
    multiples and of the first boundary of every bin level (2^17, 2^20, 2^23, 2^26), long reference skips that cross many windows, ties,
    placed reads with flag 4, unplaced reads in between.  The last four records are fixed: a 30M20000N20M across each of 2^17, 2^20 and
    2^23, and one 10M60000000N10M across 2^26, which sits in bin 0 and covers 3 663 windows"""
    rng = np.random.default_rng(seed)
    cigars = [("50M", 50), ("20M5D30M", 50), ("10M2I38M", 50), ("30M20000N20M", 50), ("1M", 1), ("25M40000N25M", 50), ("7M1D7M1I7M1D7M1I7M1D7M1I7M1D7M1I7M", 67)]
    span = {c: sum(k for k, op in bl.parse_cigar(c) if op in bl.REF_CONSUMING) for c, _ in cigars}
    lines = []
    for i in range(n - 4):
        kind = int(rng.integers(0, 12))
        if kind == 0:
            lines.append(f"u{i}\t4\t*\t0\t0\t*\t*\t0\t0\tACGTA\tIIIII")
            continue
        ref = int(rng.choice([0, 0, 0, 1, 1, 3]))
        name, L = REFS[ref]
        cigar, qlen = cigars[int(rng.integers(0, len(cigars)))]
        if span[cigar] >= L // 2:
            cigar, qlen = cigars[0]
        room = L - span[cigar]
        hot = [0, 1, room, room - 1, (1 << 14) - 1, (1 << 14) - 30, 1 << 14, (1 << 15) - 10, (1 << 26) - 1, (1 << 26) - 40, 1 << 26, (1 << 26) + 16384]
        hot += [(1 << s) + d for s in (17, 20, 23) for d in (-40, -1, 0, 16384)]
        pos = int(rng.choice(hot)) if kind < 5 else int(rng.integers(0, room + 1))
        if kind == 5:
            pos = 12345  # ties: many records with one key
        pos = min(max(pos, 0), room)
        flag = 4 if kind == 6 else 16 if kind == 7 else 0
        if flag == 4:
            cigar, qlen = "*", 7
        lines.append(f"r{i}\t{flag}\t{name}\t{pos + 1}\t30\t{cigar}\t*\t0\t0\t{'ACGTN'[i % 5] * qlen}\t{'I' * qlen}")
    for s in (17, 20, 23):
        lines.append(f"x{s}\t0\tbig\t{(1 << s) - 10000 + 1}\t30\t30M20000N20M\t*\t0\t0\t{'ACGTN' * 10}\t{'I' * 50}")
    lines.append(f"wide\t0\tbig\t{7150000 + 1}\t30\t10M60000000N10M\t*\t0\t0\t{'ACGT' * 5}\t{'I' * 20}")
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def case():
    unsorted = bl.sam_to_bam_records(synthetic_sam(), REFS)
    header = api.bgzf_compress_host(bl.bam_header("@SQ\tSN:x\tLN:1\n", REFS), eof=False)
    members, bai, rep = api.bam_sort_host(unsorted, len(REFS), bytes_in_front=len(header), report=True)
    stream, recs = sl.check_stream(members, unsorted)
    f = sl.BgzfFile(sl.compose_file(header, members))
    return {"unsorted": unsorted, "header": header, "members": members, "bai": sl.parse_bai(bai), "rep": rep, "stream": stream, "recs": recs,
            "file": f, "table": sl.member_places(f, len(header))}


def test_order_cuts_and_counters(case):
    """(check_stream ran in the fixture: the order is the stable Python sort's, the multiset is unchanged, a cut every 65 280 bytes)"""
    rep = case["rep"]
    assert rep["stream_bytes"] == len(case["stream"]) == len(case["unsorted"]) > 2 * sl.MEMBER
    assert rep["records"] == len(case["recs"]) == 1500
    assert rep["no_coor"] == sum(1 for _, r in case["recs"] if sl.fields(r)[0] < 0) > 50
    keys = [sl.sort_key(r) for _, r in case["recs"]]
    assert keys == sorted(keys) and len(set(keys)) < len(keys)


def test_index_parses_and_holds_every_property(case):
    sl.check_index(case["bai"], case["recs"], case["table"], len(REFS))
    r = case["bai"].refs
    assert r[2]["pseudo"] is None and r[2]["bins"] == [] and r[2]["linear"] == []  # a reference without records
    assert r[0]["pseudo"][3] > 0  # placed reads with flag 4 are counted apart
    levels = set(b for b, _ in r[0]["bins"])
    assert 0 in levels and any(b >= 4681 for b in levels) and any(585 <= b < 4681 for b in levels)
    assert all(any(lo <= b <= hi for b in levels) for lo, hi in sl.LEVELS), sorted(levels)  # a bin on each of the six levels
    wide = [r for _, r in case["recs"] if r[36:41] == b"wide\0"]
    assert len(wide) == 1 and sl.fields(wide[0])[3] == 0 and ((sl.fields(wide[0])[2] - 1) >> 14) - (sl.fields(wide[0])[1] >> 14) + 1 == 3663
    assert len(r[0]["linear"]) > (1 << 26) >> 14


def test_region_queries_answer_as_brute_force_does(case):
    regions = sl.edge_regions([L for _, L in REFS], np.random.default_rng(7))
    records = [r for _, r in case["recs"]]
    sl.check_queries(case["bai"], case["file"], records, regions)
    hits = [len(sl.brute(records, *q)) for q in regions]
    assert sum(1 for h in hits if h) > 100 and sum(1 for h in hits if not h) > 5  # (the regions are not all empty, nor all full)


def test_virtual_offsets_follow_the_bytes_in_front(case):
    """the same records behind another header: the same index once both are turned back into places of the stream"""
    members, bai = api.bam_sort_host(case["unsorted"], len(REFS), bytes_in_front=0)
    assert members == case["members"]
    f = sl.BgzfFile(sl.compose_file(b"", members))
    assert sl.index_in_places(sl.parse_bai(bai), sl.member_places(f, 0)) == sl.index_in_places(case["bai"], case["table"])
    assert bai != api.bam_sort_host(case["unsorted"], len(REFS), bytes_in_front=len(case["header"]))[1]


def test_known_record_starts_change_nothing_but_the_walk(case):
    """the chain walked from several known record starts at once: the same bytes; a start that is no record's is refused"""
    offs = [o for o, _ in sl.split_records(case["unsorted"])]
    want = (case["members"], api.bam_sort_host(case["unsorted"], len(REFS), bytes_in_front=len(case["header"]))[1])
    for starts in ([0], offs[::97], [offs[5], offs[5], offs[900]], [len(case["unsorted"])], offs):
        assert api.bam_sort_host(case["unsorted"], len(REFS), bytes_in_front=len(case["header"]), starts=starts) == want
    for starts in ([offs[7] + 1], [offs[9], offs[8]], [len(case["unsorted"]) + 1]):
        with pytest.raises(api.UrmapxError) as e:
            api.bam_sort_host(case["unsorted"], len(REFS), starts=starts)
        assert e.value.code == -2


def tiny(ref_id, pos, name=b"a"):
    """the shortest record: a one-letter name, no CIGAR, no bases"""
    body = struct.pack("<iiBBHHHIiii", ref_id, pos, len(name) + 1, 0, 4680 if ref_id < 0 else bl.reg2bin(pos, pos + 1), 0, 4 if ref_id < 0 else 0, 0, -1, -1, 0) + name + b"\0"
    return struct.pack("<I", len(body)) + body


@pytest.mark.parametrize("n", [0, 1, 2])
def test_few_records(n):
    unsorted = b"".join(tiny(0, 100 - i) for i in range(n))
    members, bai, rep = api.bam_sort_host(unsorted, 2, report=True)
    stream, recs = sl.check_stream(members, unsorted)
    assert rep["records"] == n and len(stream) == 38 * n and (members == b"") == (n == 0)
    f = sl.BgzfFile(sl.compose_file(b"", members))
    b = sl.parse_bai(bai)
    sl.check_index(b, recs, sl.member_places(f, 0), 2)
    assert b.n_no_coor == 0 and b.refs[1]["bins"] == []


def test_a_stream_that_ends_on_a_cut_points_at_the_end_of_file_member():
    """1020 records of 64 bytes are exactly one member: the last chunk ends where the end-of-file member begins"""
    unsorted = b"".join(tiny(0, 5 * i, b"n" * 27) for i in range(1020))
    assert len(unsorted) == sl.MEMBER
    members, bai = api.bam_sort_host(unsorted, 1, bytes_in_front=0)
    b = sl.parse_bai(bai)
    assert b.refs[0]["pseudo"][1] == len(members) << 16
    f = sl.BgzfFile(sl.compose_file(b"", members))
    recs = sl.split_records(bl.inflate(members))
    sl.check_index(b, recs, sl.member_places(f, 0), 1)
    sl.check_queries(b, f, [r for _, r in recs], [(0, 0, 1), (0, 5095, 5096), (0, 5094, 5095), (0, 0, 6000)])


def test_refusals_of_the_records():
    good = tiny(0, 5) + tiny(1, 7)
    for bad in (good[:-1],                                   # the chain runs past the end
                good + b"\x10\0\0\0" + b"\0" * 16,             # a block_size that cannot hold the core
                tiny(2, 5), tiny(-2, 5),                     # refID outside -1 .. n_ref - 1
                tiny(0, -2), tiny(1, -1),                    # a pos below -1; a reference without a pos
                good[:16] + struct.pack("<H", 60000) + good[18:]):  # a CIGAR that does not fit the record
        with pytest.raises(api.UrmapxError) as e:
            api.bam_sort_host(bad, 2)
        assert e.value.code == -2, bad[:40]  # URMAPX_E_FORMAT


# ---- urmapx_map_files with bam_sort set: the stand-alone sanitizer programs ----
@pytest.fixture(scope="module")
def san():
    if not shutil.which("g++"):
        pytest.skip("no g++ for the sanitizer builds")
    r = subprocess.run(["make", "-s", "-j3", "-C", os.path.join(ROOT, "urmap_amd", "csrc"), "san"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    return {k: os.path.join(SAN_DIR, "urmap_san_" + k) for k in ("asan", "tsan")}


SAN_ENV = dict(URX_STUB_MAP="1", ASAN_OPTIONS="exitcode=99:detect_leaks=0", UBSAN_OPTIONS="exitcode=99:halt_on_error=1", TSAN_OPTIONS="exitcode=99")


def check_sorted_file(blob, bai_bytes, unsorted_blob, option="-sort"):
    """a file of -sort against the unsorted file of the same run: header + @HD line, the oracle's order, an index that holds"""
    text, refs, _ = bl.read_bam(bl.inflate(blob))
    utext, urefs, _ = bl.read_bam(bl.inflate(unsorted_blob))
    lines, ulines = text.decode().split("\n"), utext.decode().split("\n")
    assert lines[0] == "@HD\tVN:1.6\tSO:coordinate" and refs == urefs
    assert [l for l in lines[1:] if not l.startswith("@PG")] == [l for l in ulines if not l.startswith("@PG")]
    pg = [l for l in lines if l.startswith("@PG")]
    assert len(pg) == 1 and (option is None or option in pg[0])
    f = sl.BgzfFile(blob)
    first = f.members()[0]
    in_front = f.member(first[0])[1]  # the header block has a member of its own
    head_len = first[1]
    inflated = bl.inflate(blob)
    unsorted_stream = bl.inflate(unsorted_blob)[len(bl.bam_header(utext, urefs)):]
    assert blob.endswith(api.BGZF_EOF)
    members = blob[in_front:len(blob) - len(api.BGZF_EOF)]
    stream, recs = sl.check_stream(members, unsorted_stream)
    assert inflated[head_len:] == stream
    b = sl.parse_bai(bai_bytes)
    sl.check_index(b, recs, sl.member_places(f, in_front), len(refs))
    return inflated, b, f, recs, refs


@pytest.mark.parametrize("build,extra", [("asan", []), ("asan", ["-batch", "64", "-streams", "3"]), ("asan", ["-2"]), ("tsan", ["-batch", "64", "-streams", "3"])])
def test_pipeline_sort_under_sanitizers(tmp_path, san, build, extra):
    paired = "-2" in extra
    fq = os.path.join(GOLD, "pe150_1.fq" if paired else "se150.fq")
    extra = (["-2", os.path.join(GOLD, "pe150_2.fq")] if paired else extra) + ["-biglen", "500000000"]
    env = dict(os.environ, **SAN_ENV)
    plain, out = str(tmp_path / "u.bam"), str(tmp_path / "s.bam")
    for path, flag in ((plain, ["-bam"]), (out, ["-bam", "-sort"])):
        r = subprocess.run([san[build], "map", fq, "-o", path] + extra + flag, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    assert not os.path.exists(plain + ".bai")
    inflated, b, f, recs, refs = check_sorted_file(open(out, "rb").read(), open(out + ".bai", "rb").read(), open(plain, "rb").read(),
                                                    option=None)  # (the stand-alone program writes no command line into @PG)
    assert len(recs) >= 400
    records = [r for _, r in recs]
    sl.check_queries(b, f, records, sl.edge_regions([L for _, L in refs], np.random.default_rng(3), 60))
    # the inflated bytes do not depend on how the work was cut
    if build == "asan" and not paired and extra[0] != "-batch":
        for other in (["-batch", "50"], ["-streams", "1"], ["-threads", "3"]):
            r = subprocess.run([san[build], "map", fq, "-o", out + "2", "-bam", "-sort"] + extra + other, env=env, capture_output=True, text=True)
            assert r.returncode == 0, r.stdout + r.stderr
            assert bl.inflate(open(out + "2", "rb").read()) == inflated, other


def test_refusals_of_the_options(tmp_path, san):
    fq = os.path.join(GOLD, "se150.fq")
    env = dict(os.environ, **SAN_ENV)
    out = str(tmp_path / "no.bam")
    for args, word in ((["-sort"], "bam"), (["-bam", "-sort", "-shards", "2"], "shard"), (["-bam", "-sort", "-null"], "discard")):
        r = subprocess.run([san["asan"], "map", fq, "-o", out] + args, env=env, capture_output=True, text=True)
        assert "rc=-5" in r.stdout and word in r.stdout, r.stdout + r.stderr
        assert not os.path.exists(out) and not os.path.exists(out + ".bai") and not os.path.exists(out + ".0")
