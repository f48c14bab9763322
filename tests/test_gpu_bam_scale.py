"""GPU tests of the BAM family at genome-scale coordinates: the device sort's index kernels (bounds, lin, bin_key, chunk_flag,
chunk_write in bam_sort.hip) on records that crowd every level boundary of the BAI bins up to 2^26 and on records at and beyond 2^29,
the depth kernels around 2^26 columns, and -- on the islands fixture of tests/islands_lib.py, a genome of 2^26 + 40 000 bases that is N
but for islands around each boundary -- the record kernel's bins, the reference fetches of the tag kernels above 2^26 of the sequence
store, and the whole road from FASTQ to a sorted, marked, indexed BAM file with its depth."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_lib as bl
import bam_sort_lib as sl
import depth_lib as dl
import islands_lib as il
import markdup_lib as ml
import tags_lib as tl
from test_bam_scale_cpu import BEYOND_REFS, beyond_records, check_beyond
from test_bam_sort_cpu import REFS, synthetic_sam
from test_gpu_bam_sort import both
from test_gpu_bam_sort_external import external
from test_gpu_depth import SEGMENT, device_host_model, spans

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "urmap_amd", "urmap")
KNOBS = ("URMAPX_TEST_SORT_STAGE", "URMAPX_TEST_SORT_PARTITION", "URMAPX_TEST_SORT_SLICE", "URMAPX_TEST_DEPTH_SLICE", "URMAPX_HOST_TEXT")
RG_ID = "isl.1"
LENGTHS = [L for _, L in REFS]


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def levels_of(bai, ref=0):
    return set(il.level_of(b) for b, _ in bai.refs[ref]["bins"])


# ---- synthetic records through the device sort ----
@pytest.fixture(scope="module")
def synthetic():
    from urmap_amd import api
    records = bl.sam_to_bam_records(synthetic_sam(), REFS)
    hm, hbai = api.bam_sort_host(records, len(REFS), bytes_in_front=555)
    f = sl.BgzfFile(b"\0" * 555 + hm + api.BGZF_EOF)
    return {"records": records, "stream": bl.inflate(hm), "places": sl.index_in_places(sl.parse_bai(hbai), sl.member_places(f, 555)),
            "regions": sl.edge_regions(LENGTHS, np.random.default_rng(7), 60)}


def check_own_index(b, f, table, stream, regions, n_ref):
    """the device's own .bai against the yardstick: every property of the index, and what a reader finds through it"""
    recs = sl.split_records(stream)
    sl.check_index(b, recs, table, n_ref)
    sl.check_queries(b, f, [r for _, r in recs], regions)


@pytest.mark.parametrize("road", ["in core", "external", "markdup"])
def test_synthetic_records_through_the_device_sort(monkeypatch, synthetic, road):
    """1 500 records on a reference of 2^26 + 90 000 with positions on both sides of 2^14, 2^17, 2^20, 2^23 and 2^26, skips across each
    and one record of 3 663 windows in bin 0: the device's stream and index are the host's, and the device's own .bai holds"""
    from urmap_amd import api
    records, n_ref = synthetic["records"], len(REFS)
    if road == "in core":
        stream, b, f, table, rep = both(records, n_ref, in_front=555)
        sl.check_stream(f.blob[555:-len(api.BGZF_EOF)], records)
    elif road == "external":
        monkeypatch.setenv("URMAPX_TEST_SORT_SLICE", "1")
        stream, places, rep, f, b, table = external(monkeypatch, records, n_ref, 1, 4096, in_front=555)
        assert rep["external"] == 1 and rep["partitions"] == -(-len(records) // sl.MEMBER) > 2 and rep["stage_chunks"] > 20
        assert stream == synthetic["stream"] and places == synthetic["places"]
    else:
        dm, dbai, rep = api.bam_sort(records, n_ref, device=0, bytes_in_front=555, report=True, markdup=True)
        hm, hbai = api.bam_sort_host(records, n_ref, bytes_in_front=555, markdup=True)
        stream = bl.inflate(dm)
        assert stream == bl.inflate(hm)
        ml.check(records, stream, synthetic["stream"], rep)
        assert rep["fragments_duplicate"] > 100
        f, fh = sl.BgzfFile(b"\0" * 555 + dm + api.BGZF_EOF), sl.BgzfFile(b"\0" * 555 + hm + api.BGZF_EOF)
        b, table = sl.parse_bai(dbai), sl.member_places(f, 555)
        assert sl.index_in_places(b, table) == sl.index_in_places(sl.parse_bai(hbai), sl.member_places(fh, 555)) == synthetic["places"]
    check_own_index(b, f, table, stream, synthetic["regions"], n_ref)
    assert levels_of(b) == {0, 1, 2, 3, 4, 5} and len(b.refs[0]["linear"]) > (1 << 26) >> 14


def test_long_spans_at_neighbouring_positions_contend_for_the_windows():
    """3 000 records that each span more than 2 000 windows, at neighbouring positions: lin_kernel's atomicMin under contention"""
    lines = []
    for i in range(3000):
        pos = 5000 + 3 * ((i * 7) % 64) + (16384 * 37 if i % 500 == 499 else 0)
        skip = 40000000 - 16384 * (i % 3)
        lines.append(f"c{i}\t0\tbig\t{pos + 1}\t9\t10M{skip}N10M\t*\t0\t0\t{'ACGT'[i % 4] * 20}\t{'F' * 20}")
    records = bl.sam_to_bam_records("\n".join(lines) + "\n", REFS)
    assert min((sl.fields(r)[2] - 1 >> 14) - (sl.fields(r)[1] >> 14) + 1 for _, r in sl.split_records(records)[:10]) > 2000
    stream, b, f, table, rep = both(records, len(REFS))
    sl.check_index(b, sl.split_records(stream), table, len(REFS))
    assert len(b.refs[0]["linear"]) > 2400 and [bin_ for bin_, _ in b.refs[0]["bins"]] == [1]


# ---- beyond 2^29 ----
@pytest.mark.parametrize("road", ["in core", "external"])
def test_beyond_2_29_the_device_index_is_the_hosts_and_well_formed(monkeypatch, road):
    from urmap_amd import api
    records, n_ref = beyond_records(), len(BEYOND_REFS)
    if road == "in core":
        both(records, n_ref, in_front=321)
        dm, dbai = api.bam_sort(records, n_ref, device=0, bytes_in_front=321)
    else:
        monkeypatch.setenv("URMAPX_TEST_SORT_SLICE", "1")
        monkeypatch.setenv("URMAPX_TEST_SORT_PARTITION", "1")
        monkeypatch.setenv("URMAPX_TEST_SORT_STAGE", "1000")
        dm, dbai, rep = api.bam_sort(records, n_ref, device=0, bytes_in_front=321, budget=0, report=True)
        assert rep["external"] == 1 and rep["stage_chunks"] > 3
        hm, hbai = api.bam_sort_host(records, n_ref, bytes_in_front=321)
        assert bl.inflate(dm) == bl.inflate(hm)
        fd, fh = sl.BgzfFile(b"\0" * 321 + dm + api.BGZF_EOF), sl.BgzfFile(b"\0" * 321 + hm + api.BGZF_EOF)
        assert sl.index_in_places(sl.parse_bai(dbai), sl.member_places(fd, 321)) == sl.index_in_places(sl.parse_bai(hbai), sl.member_places(fh, 321))
    check_beyond(dm, dbai, records, in_front=321)


# ---- depth at 2^26 columns ----
def test_depth_around_the_level_boundaries_and_segments_above_2_25():
    """one reference of 2^26 + 90 000 columns: spans across, up to and from every level boundary of the bins and multiples of the run
    search's segment above 2^25, the last column, spans that hang over the end"""
    L = (1 << 26) + 90000
    at = [1 << s for s in (14, 17, 20, 23, 26)] + [k * SEGMENT for k in (16, 17, 24, 31, 32)] + [L]
    assert all(a % SEGMENT == 0 for a in at[5:10]) and at[6] > 1 << 25 and at[9] == 1 << 26
    pos, length = [], []
    for a in at:
        for p, n in ((a - 5, 10), (a - 1, 1), (a, 1), (a - 70, 70), (a, 3), (a - 200, 150), (a - 1, 2)):
            pos.append(p)
            length.append(n)
    pos += [0, 0, L - 1, (1 << 26) - 30000]
    length += [1, 40, 1, 60000]
    text, runs, summ, rep = device_host_model(spans(np.zeros(len(pos), dtype=int), pos, length), ["big"], [L])
    dl.check_tiling(text, ["big"], [L])
    rows = dl.parse(text)
    assert rows[-1][2] == L and runs == len(rows) > 60
    assert summ[0]["covered"] > 60000 and any(b < 1 << 26 < e and d > 0 for _, b, e, d in rows)


# ---- the islands ----
@pytest.fixture(scope="module")
def islands(tmp_path_factory):
    from urmap_amd import api
    out = il.build(tmp_path_factory.mktemp("islands"))
    out["index"] = api.Index.open(out["ufi"]).upload(0)
    out["mapper"] = api.Mapper(out["index"], device=0)
    assert [(n, l) for n, l, _ in out["index"].directory()] == out["refs"] and out["index"].directory()[1][2] > 1 << 26
    for kind in ("se", "pe"):
        sam = os.path.join(out["dir"], kind + ".oracle.sam")
        if kind == "se":
            out["oracle"].map_file_se(out["fq_se"], sam)
        else:
            out["oracle"].map_file_pe(out["fq_1"], out["fq_2"], sam)
        out["sam_" + kind] = open(sam, "rb").read()
    yield out
    out["mapper"].close()


def fastq_of(islands, kind):
    return [open(islands[k], "rb").read() for k in (("fq_se",) if kind == "se" else ("fq_1", "fq_2"))]


def bam_text(m, fq, tags, rg):
    """the text stage's raw BAM records of one chunk of FASTQ text"""
    from urmap_amd import api
    m.set_tags(tags, rg)
    m.set_bam(True)
    try:
        out, rep = m.map_text_se(fq[0]) if len(fq) == 1 else m.map_text_pe(*fq)
    finally:
        m.set_bam(False)
        m.set_tags(0, None)
    assert rep["reason"] == api.TEXT_OK and rep["sam_bytes"] == len(out), rep
    return out


def check_fields(records, islands, want_lines, rg):
    """every record: bam_lib accepts its bin, without the fields it is the oracle's SAM line, NM and MD are the yardstick's from the FASTA"""
    got = tl.read_bam_records_aux(records, islands["refs"])
    assert [line for line, _ in got] == want_lines
    above = 0
    for line, aux in got:
        f = line.split("\t")
        tags = {t: v for t, _, v in aux}
        assert tags.pop("RG", None) == rg
        if f[2] == "*":
            assert not tags
            continue
        assert (tags["NM"], tags["MD"]) == tl.calmd(islands["text"][f[2]], int(f[3]), f[5], f[9]), line[:80]
        assert [t for t, _, _ in aux][:3] == ["NM", "MD", "AS"]
        above += f[2] == "small" or int(f[3]) > 1 << 26
    assert above >= 10  # (windows fetched above 2^26 of the sequence store)


@pytest.mark.parametrize("kind", ["se", "pe"])
def test_islands_text_stage_equals_the_host_formatters(islands, kind):
    from urmap_amd import api
    m, idx, paired = islands["mapper"], islands["index"], kind == "pe"
    fq = fastq_of(islands, kind)
    sets = [api.read_fastq_arrays(islands[k]) for k in (("fq_se",) if not paired else ("fq_1", "fq_2"))]
    labels, bases, offs, quals = sets[0] if not paired else api.interleave_pairs(*sets)
    res, ops = m.map_pe(bases, offs) if paired else m.map_se(bases, offs)
    reads = islands["se"] if not paired else [x for p in islands["pe"] for x in p]
    for r, o in zip(reads, res):  # the device maps every read where it was drawn from
        assert (int(o["seq_index"]), int(o["coord"]), bool(o["plus"])) == (r.ref, r.pos, r.plus) if r.ref is not None else o["dbpos"] == il.UNMAPPED, r.label
    want_lines = bl.sam_records(islands["sam_" + kind])
    plain = bam_text(m, fq, 0, None)
    assert plain == (idx.bam_pe if paired else idx.bam_se)(res, ops, labels, bases, offs, quals) == bl.sam_to_bam_records(islands["sam_" + kind], islands["refs"])
    assert bl.read_bam_records(plain, islands["refs"]) == want_lines  # (every bin is reg2bin of its record)
    bins = [struct.unpack_from("<H", r, 14)[0] for _, r in sl.split_records(plain) if struct.unpack_from("<i", r, 4)[0] == 0]
    assert set(il.level_of(b) for b in bins) == {0, 1, 2, 3, 4, 5} and {585 + 511, 73 + 63, 9 + 7} <= set(bins)  # (and the upper levels' last bins)
    tagged =bam_text(m, fq, api.TAG_ALL, RG_ID)
    assert tagged == idx.records_tags(res, ops, labels, bases, offs, quals, tags=api.TAG_ALL, rg_id=RG_ID, bam=True, paired=paired)
    check_fields(tagged, islands, want_lines, RG_ID)
    # 64 records a chunk, then chunks that begin one read later: boundary-crossing records on other lanes of the wavefront
    lines = [f.split(b"\n")[:-1] for f in fq]
    n = len(lines[0]) // 4
    per = 64 if not paired else 32
    for first in (0, 1):
        cuts = sorted(set([0] + list(range(first, n, per)) + [n]))
        got = b"".join(bam_text(m, [b"\n".join(l[4 * a:4 * stop]) + b"\n" for l in lines], api.TAG_ALL, RG_ID) for a, stop in zip(cuts, cuts[1:]))
        assert got == tagged, first


def without_aux(rec):
    """a record cut off behind its qualities, block_size set to match"""
    l_name, n_cig, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    core = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    return struct.pack("<I", core) + rec[4:4 + core]


def opened_file(path):
    """a sorted BAM file and its index -> (inflated bytes, header length, record stream, [(offset, record)], the file, the places, the index)"""
    from urmap_amd import api
    blob = open(path, "rb").read()
    assert blob.endswith(api.BGZF_EOF)
    inflated = bl.inflate(blob)
    text, refs, _, stream = tl.read_bam_aux(inflated)  # (bam_lib reads the header and every record: each bin is reg2bin)
    f = sl.BgzfFile(blob)
    in_front = f.member(0)[1]  # the header block has a member of its own
    assert f.members()[0][1] == len(inflated) - len(stream) and text.startswith(b"@HD\tVN:1.6\tSO:coordinate\n")
    table = sl.member_places(f, in_front)
    return inflated, refs, stream, sl.split_records(stream), f, table, sl.parse_bai(open(path + ".bai", "rb").read())


@pytest.fixture(scope="module")
def island_files(islands):
    """per kind: the unsorted file of the records with their fields, then -sort -markdup -depth on the device"""
    from urmap_amd import api
    out = {}
    for kind in ("se", "pe"):
        fq = [islands["fq_se"], None] if kind == "se" else [islands["fq_1"], islands["fq_2"]]
        path = lambda k, ext, kind=kind: os.path.join(islands["dir"], f"{kind}_{k}.{ext}")  # noqa: E731
        api.map_files(islands["index"], fq[0], fq[1], samout=path("plain", "bam"), bam=True, tags=api.TAG_ALL)
        rep = api.map_files(islands["index"], fq[0], fq[1], samout=path("dev", "bam"), bam=True, bam_sort=True, markdup=True,
                            depth_out=path("dev", "bedgraph"), tags=api.TAG_ALL)
        out[kind] = {"fq": fq, "path": path, "rep": rep, "unsorted": tl.read_bam_aux(bl.inflate(open(path("plain", "bam"), "rb").read()))[3]}
    return out


@pytest.mark.parametrize("kind", ["se", "pe"])
def test_islands_file_to_file(monkeypatch, islands, island_files, kind):
    from urmap_amd import api
    c = island_files[kind]
    path, unsorted = c["path"], c["unsorted"]
    inflated, refs, stream, recs, f, table, b = opened_file(path("dev", "bam"))
    assert refs == islands["refs"]
    # the records: without the duplicate bit and the fields, the oracle's SAM; the order is the stable sort of the unsorted file's
    want = [r for _, r in sl.split_records(bl.sam_to_bam_records(islands["sam_" + kind], refs))]
    assert sorted(without_aux(r) for _, r in sl.split_records(ml.mask_dup(stream))) == sorted(want)
    assert [r for _, r in sl.split_records(ml.mask_dup(stream))] == sl.oracle_order([r for _, r in sl.split_records(ml.mask_dup(unsorted))])
    check_fields(stream, islands, [bl.normalise_sam_line(l) for l in bl.read_bam_records(b"".join(without_aux(r) for _, r in recs), refs)], None)
    # the flags are the model's
    came = [r for _, r in sl.split_records(unsorted)]
    flagged, counters = ml.model(came)
    order = sorted(range(len(came)), key=lambda i: sl.sort_key(came[i]))
    assert [bool(x & 0x400) for x in ml.flags_of(stream)] == [flagged[i] for i in order] and sum(flagged) >= 5
    # the index, and what a reader finds through it
    sl.check_index(b, recs, table, len(refs))
    sl.check_queries(b, f, [r for _, r in recs], sl.edge_regions([L for _, L in refs], np.random.default_rng(5), 60))
    assert levels_of(b) == {0, 1, 2, 3, 4, 5} and len(b.refs[0]["linear"]) > 4096
    # the depth of the file's own records
    names, lens = [n for n, _ in refs], [L for _, L in refs]
    depth = open(path("dev", "bedgraph"), "rb").read()
    assert depth == dl.model(stream, names, lens)[0]
    assert any(beg < 1 << 26 < end and d > 0 for _, beg, end, d in dl.parse(depth))
    # the host's road: the same inflated bytes, the same index in places of the stream, the same depth
    monkeypatch.setenv("URMAPX_HOST_TEXT", "1")
    api.map_files(islands["index"], c["fq"][0], c["fq"][1], samout=path("host", "bam"), bam=True, bam_sort=True, markdup=True,
                  depth_out=path("host", "bedgraph"), tags=api.TAG_ALL)
    hinflated, _, _, _, hf, htable, hb = opened_file(path("host", "bam"))
    assert hinflated == inflated and sl.index_in_places(hb, htable) == sl.index_in_places(b, table)
    assert open(path("host", "bedgraph"), "rb").read() == depth


def test_islands_through_the_executable(islands, island_files):
    """urmap -map2 ... -bamout -sort -markdup -depth -tags: the records, the index and the depth file of the library call"""
    c = island_files["pe"]
    out, bed = c["path"]("cli", "bam"), c["path"]("cli", "bedgraph")
    r = subprocess.run([EXE, "-map2", islands["fq_1"], "-reverse", islands["fq_2"], "-ufi", islands["ufi"], "-quiet", "-bamout", out, "-sort", "-markdup",
                        "-depth", bed, "-tags", "NM,MD,AS"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    _, refs, stream, recs, f, table, b = opened_file(out)
    _, _, want_stream, _, wf, wtable, wb = opened_file(c["path"]("dev", "bam"))
    assert stream == want_stream and sl.index_in_places(b, table) == sl.index_in_places(wb, wtable)
    sl.check_index(b, recs, table, len(refs))
    assert open(bed, "rb").read() == open(c["path"]("dev", "bedgraph"), "rb").read()
