"""The BAM family at genome-scale coordinates, host side: the islands fixture's check of itself (tests/islands_lib.py), the host
formatters at every level boundary of the BAI bins against bam_lib's reading of the oracle's SAM text, and the contract of the sorted
output for records at and beyond 2^29, where the BAI scheme ends (include/urmapx.h "Sorted BAM output")."""
import struct

import numpy as np
import pytest

import bam_lib as bl
import bam_sort_lib as sl
import islands_lib as il
import tags_lib as tl
from test_abi_cpu import oracle_results_as_product
from urmap_amd import api

E29 = 1 << 29


@pytest.fixture(scope="module")
def islands(tmp_path_factory):
    return il.build(tmp_path_factory.mktemp("islands"))


def arrays_of(islands, paired):
    if paired:
        return api.interleave_pairs(api.read_fastq_arrays(islands["fq_1"]), api.read_fastq_arrays(islands["fq_2"]))
    return api.read_fastq_arrays(islands["fq_se"])


def oracle_maps(islands, paired):
    """-> (the product's result arrays made of the oracle's hits, the FASTQ arrays, the oracle's results)"""
    labels, bases, offs, quals = arrays_of(islands, paired)
    ores, opaths, _ = islands["oracle"].map_pe(bases, offs) if paired else islands["oracle"].map_se(bases, offs)
    res, ops = oracle_results_as_product(ores, opaths)
    return (res, ops, labels, bases, offs, quals), ores


def check_drawn(reads, ores):
    """every read maps where it was drawn from; the ones from nowhere do not map"""
    assert len(reads) == len(ores)
    for r, o in zip(reads, ores):
        if r.ref is None:
            assert o["dbpos"] == il.UNMAPPED, r.label
        else:
            assert (int(o["seq_index"]), int(o["coord"]), bool(o["plus"])) == (r.ref, r.pos, r.plus), (r.label, o)


# ---- the fixture checks itself ----
def test_the_islands_are_where_the_tests_need_them(islands):
    big = islands["genome"][0][1]
    assert len(big) == (1 << 26) + 40000 and islands["refs"] == [("big", len(big)), ("small", 30000)]
    for e in il.EDGES:
        assert ord("N") not in big[e - 1000:e + 1000] and big[e - 1001] == big[e + 1000] == ord("N")
    assert ord("N") not in big[:1500] and ord("N") not in big[-1500:] and big[1500] == big[-1501] == ord("N")
    for e in il.LAST_EDGES:
        assert ord("N") not in big[e - 1000:e + 1000] and big[e - 1001] == big[e + 1000] == ord("N")
    assert int((big != ord("N")).sum()) == 8 * 2000 + 2 * 1500
    d = islands["oracle"].directory()
    assert [(n, l) for n, l, _ in d] == islands["refs"] and d[1][2] > 1 << 26  # small lies above 2^26 in the sequence store
    assert 200 <= len(islands["se"]) + 2 * len(islands["pe"]) <= 600


def test_every_island_read_maps_where_it_was_drawn_from(islands):
    _, ores = oracle_maps(islands, False)
    check_drawn(islands["se"], ores)
    plain = [o for r, o in zip(islands["se"], ores) if r.ref is not None and not r.mutated]
    assert len(plain) > 40 and all(o["mapq"] == 40 for o in plain)
    _, pres = oracle_maps(islands, True)
    check_drawn([m for p in islands["pe"] for m in p], pres)
    # the mapped set holds a record on each of the six bin levels, for single reads and for pairs: a later change to the generator
    # cannot quietly take the level boundaries out of the tests that use it
    for reads in (islands["se"], [m for p in islands["pe"] for m in p]):
        levels = set(il.level_of(bl.reg2bin(r.pos, r.pos + r.span)) for r in reads if r.ref == 0)
        assert levels == {0, 1, 2, 3, 4, 5}, levels
    # and, across the last boundaries below 2^26, the last bin of each upper level that a reference of this length has
    for reads in (islands["se"], [m for p in islands["pe"] for m in p]):
        assert {585 + 511, 73 + 63, 9 + 7, 1, 0} <= set(bl.reg2bin(r.pos, r.pos + r.span) for r in reads if r.ref == 0)
    first = {e: bl.reg2bin(e - 150, e) for e in il.EDGES}  # a read that ends exactly at the boundary stays on the child level
    assert all(b >= 4681 for b in first.values())
    assert sum(1 for r in islands["se"] if r.ref == 0 and r.pos + r.span in il.EDGES) >= 10
    assert sum(1 for r in islands["se"] if r.ref == 0 and r.pos in il.EDGES) >= 10
    assert any(r.pos == 0 for r in islands["se"]) and any(r.ref == 0 and r.pos + r.span == il.BIG for r in islands["se"])


# ---- the host formatters at the island coordinates ----
def check_tagged(tagged, plain_lines, ores, islands):
    """BAM records with NM, MD, AS: without the fields they are the plain lines; the fields are the yardstick's, read off the FASTA"""
    got = tl.read_bam_records_aux(tagged, islands["refs"])
    assert len(got) == len(plain_lines) == len(ores)
    for (line, aux), want, o in zip(got, plain_lines, ores):
        assert line == want
        f = line.split("\t")
        if f[2] == "*":
            assert aux == []
            continue
        nm, md = tl.calmd(islands["text"][f[2]], int(f[3]), f[5], f[9])
        assert aux == [("NM", tl.smallest_int_type(nm), nm), ("MD", "Z", md), ("AS", tl.smallest_int_type(int(o["score"])), int(o["score"]))], line[:80]


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_host_formatters_equal_the_oracles_sam_in_bam(islands, tmp_path, paired):
    arrays, ores = oracle_maps(islands, paired)
    sam = str(tmp_path / "oracle.sam")
    if paired:
        islands["oracle"].map_file_pe(islands["fq_1"], islands["fq_2"], sam)
    else:
        islands["oracle"].map_file_se(islands["fq_se"], sam)
    text = open(sam, "rb").read()
    idx = api.Index.open(islands["ufi"])
    try:
        got = idx.bam_pe(*arrays) if paired else idx.bam_se(*arrays)
        assert got == bl.sam_to_bam_records(text, islands["refs"])
        lines = bl.read_bam_records(got, islands["refs"])  # (asserts bin == reg2bin of every record)
        assert lines == bl.sam_records(text)
        bins = [struct.unpack_from("<H", r, 14)[0] for _, r in sl.split_records(got) if struct.unpack_from("<i", r, 4)[0] == 0]
        assert set(il.level_of(b) for b in bins) == {0, 1, 2, 3, 4, 5}
        if paired:
            f = [l.split("\t") for l in lines]
            assert any(int(x[3]) <= 1 << 26 < int(x[7]) and int(x[8]) > 0 for x in f)  # next_pos beyond 2^26, TLEN across it
        check_tagged(idx.records_tags(*arrays, tags=api.TAG_ALL, bam=True, paired=paired), lines, ores, islands)
    finally:
        idx.close()


# ---- the contract beyond 2^29 ----
BEYOND_REFS = [("huge", (1 << 31) - 1), ("empty", 1000), ("other", 100000)]


def beyond_records():
    """records at and beyond the end of the BAI scheme among ordinary ones of the same reference, a second reference and unplaced ones"""
    L = []

    def rec(name, ref, pos, cigar="40M", flag=0):
        qlen = sum(n for n, op in bl.parse_cigar(cigar) if op in "MIS=X") if cigar != "*" else 7
        L.append(f"{name}\t{flag}\t{ref}\t{pos + 1}\t30\t{cigar}\t*\t0\t0\t{'ACGT'[len(L) % 4] * qlen}\t{'I' * qlen}")

    for k, pos in enumerate((E29 - 1, E29, E29 + 16384 + 5, (1 << 30) + 5, (1 << 31) - 1)):
        rec(f"one{k}", "huge", pos, "1M")
    rec("begins_below", "huge", E29 - 20, "50M")
    rec("skips_beyond", "huge", E29 - 30000, "25M40000N25M")
    rec("collision_twice", "huge", E29 + 16384 + 5, "30M")
    rec("collision_flag4", "huge", E29 + 16384 + 9, "*", flag=4)
    rec("far", "huge", (1 << 30) + 5, "20M2D20M")
    rec("ends_at", "huge", E29 - 40, "40M")       # the last base is 2^29 - 1
    rec("last_window", "huge", E29 - 16384, "40M")
    for k, pos in enumerate((0, 100, 16383, 20000, (1 << 26) - 10, (1 << 26) + 5, (1 << 28) + 77, E29 - 70000, E29 - 16390)):
        rec(f"plain{k}", "huge", pos)
        rec(f"again{k}", "huge", pos, "10M5D30M", flag=16)
    for k in range(12):
        rec(f"other{k}", "other", 7000 * k, "30M20000N20M" if k % 3 == 0 else "50M")
    for k in range(5):
        L.insert(3 + 7 * k, f"unplaced{k}\t4\t*\t0\t0\t*\t*\t0\t0\tACGTA\tIIIII")
    order = np.random.default_rng(29).permutation(len(L))
    return bl.sam_to_bam_records("\n".join(L[i] for i in order) + "\n", BEYOND_REFS)


BEYOND_REGIONS = [(0, 0, 1), (0, 0, 30000), (0, (1 << 26) - 100, (1 << 26) + 100), (0, E29 - 100000, E29), (0, E29 - 100, E29), (0, E29 - 1, E29),
                  (0, E29 - 30000, E29 - 29990), (0, E29 - 16384, E29 - 16383), (0, E29 - 41, E29 - 39), (0, 0, E29), (0, 1 << 28, E29 - 20000),
                  (2, 0, 100000), (2, 6999, 7001), (2, 20000, 27030), (1, 0, 1000)]


def check_beyond(members, bai_bytes, unsorted, in_front=0):
    """the yardstick's checks of a sorted stream and its index for the records of beyond_records(); -> the parsed index"""
    stream, recs = sl.check_stream(members, unsorted)  # the order is the stable Python sort's
    f = sl.BgzfFile(b"\0" * in_front + members + api.BGZF_EOF)
    b = sl.parse_bai(bai_bytes)  # (no bin above 37 448 but the pseudo-bin, which comes once; at most 32 768 windows)
    sl.check_index(b, recs, sl.member_places(f, in_front), len(BEYOND_REFS))
    sl.check_queries(b, f, [r for _, r in recs], BEYOND_REGIONS)
    huge = b.refs[0]
    placed = [sl.fields(r) for _, r in recs if sl.fields(r)[0] == 0]
    beyond = sum(1 for p in placed if p[1] >= E29)
    assert beyond == 7 and huge["pseudo"][2] + huge["pseudo"][3] == len(placed) and huge["pseudo"][3] == 1
    assert len(huge["linear"]) == 32768 and b.n_no_coor == 5
    assert max(bin_ for bin_, _ in huge["bins"]) == sl.MAX_BIN
    return b


def test_the_index_is_well_formed_whatever_lies_beyond_2_29():
    unsorted = beyond_records()
    members, bai = api.bam_sort_host(unsorted, len(BEYOND_REFS), bytes_in_front=321)
    b = check_beyond(members, bai, unsorted, in_front=321)
    hits = [len(sl.brute([r for _, r in sl.split_records(unsorted)], *q)) for q in BEYOND_REGIONS]
    assert hits[4] >= 4 and hits[5] >= 3 and hits[-1] == 0  # (the regions at the end of the scheme are not empty)
    # the records beyond are in no chunk: the chunks' bytes are those of the records below 2^29
    recs = sl.split_records(bl.inflate(members))
    below = sum(len(r) for _, r in recs if sl.fields(r)[3] is not None)
    f = sl.BgzfFile(b"\0" * 321 + members + api.BGZF_EOF)
    refs, _ = sl.index_in_places(b, sl.member_places(f, 321))
    assert sum(y - x for r in refs for _, cs in r["bins"] for x, y in cs) == below
