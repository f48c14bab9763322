"""CPU: the depth rule (include/urmapx.h "Depth").  urmapx_bam_depth_host against the model of tests/depth_lib.py on hand-made records,
the struct layouts and the memory sum, the host twin of the sort with depth, and -- through the stand-alone sanitizer program -- the
refusals of the options and the depth file written beside a sorted, marked BAM file."""
import ctypes as C
import os
import stat
import subprocess

import pytest

import bam_lib as bl
import bam_sort_lib as sl
import depth_lib as dl
import markdup_lib as ml
from test_bam_sort_cpu import tiny
from test_markdup_cpu import Q, pair, with_copies
from test_sanitizers_cpu import run as san_run, san  # noqa: F401  (san is a fixture: it builds the programs)
from urmap_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
R = dl.R


def agree(got, want):
    assert got[0] == want[0], (got[0][:300], want[0][:300])
    assert got[1] == want[1] and got[2] == want[2]


def host_equals_model(records, names, lens, min_mapq=0):
    got = api.bam_depth_host(records, len(lens), names, lens, min_mapq=min_mapq)
    agree(got, dl.model(records, names, lens, min_mapq))
    dl.check_tiling(got[0], names, lens)
    return got


def test_no_records_at_all():
    text, runs, refs = host_equals_model(b"", ["a", "bb"], [7, 3])
    assert text == b"a\t0\t7\t0\nbb\t0\t3\t0\n" and runs == 2 and refs == [dict(reads=0, covered=0, bases=0, mapq_sum=0)] * 2
    assert api.bam_depth_host(b"", 0, [], []) == (b"", 0, [])


def test_one_record():
    text, runs, refs = host_equals_model(dl.with_mapq(R(1, 2, 0, "3M", b""), 40), ["a", "bb"], [7, 9])
    assert text == b"a\t0\t7\t0\nbb\t0\t2\t0\nbb\t2\t5\t1\nbb\t5\t9\t0\n"
    assert refs[1] == dict(reads=1, covered=3, bases=3, mapq_sum=40)


@pytest.mark.parametrize("min_mapq", [0, 17, 18, 61, 255])
def test_every_op_edge_flag_and_name(min_mapq):
    """dl.cigar_cases: every CIGAR op, a record that starts with D, one with only S and I, ends at and beyond l_ref, the sentinel entry
    between two references, references of length 0 and 1, each excluded flag alone, names of 1 and 200 characters; min_mapq at 0, at one
    record's MAPQ (17), one above it, and above the others"""
    records, names, lens = dl.cigar_cases()
    text, runs, refs = host_equals_model(records, names, lens, min_mapq)
    rows = dl.parse(text)
    assert not any(n == b"zero" for n, _, _, _ in rows)
    assert ((b"n" * 200, 0, 299, 1) if min_mapq == 0 else (b"n" * 200, 0, 300, 0)) in rows
    if min_mapq == 0:
        assert (b"c", 15, 22, 0) in rows and (b"c", 22, 41, 1) in rows       # 5M to 15, then 3D 4N skipped, then 9= 10X as one run
        assert (b"c", 0, 4, 0) in rows and (b"c", 4, 15, 1) in rows           # 4D6M at pos 0 meets the 5M at 10: one run
        assert (b"c", 395, 400, 2) in rows and (b"one", 0, 1, 2) in rows      # the clipped ends; the one-column reference
        assert refs[0]["reads"] == 6 and refs[2] == dict(reads=3, covered=1, bases=2, mapq_sum=0)
        assert (b"last", 30, 40, 3) in rows                                   # 0x800, 0x10 and 0x41 count; 0x4, 0x100, 0x200, 0x400 do not
    want45 = {0: 5, 17: 4, 18: 3, 61: 1, 255: 1}[min_mapq]
    assert (b"last", 45, 48, want45) in rows


@pytest.mark.parametrize("depth", [5, 12, 100000])
def test_depths_of_one_two_and_six_digits(depth):
    records, names, lens = dl.digits_case(depth)
    text, runs, refs = host_equals_model(records, names, lens)
    assert text == b"d\t0\t5\t0\nd\t5\t25\t%d\nd\t25\t30\t0\n" % depth and refs[0]["bases"] == 20 * depth


def test_refusals_of_the_arguments():
    for names in (["a", ""], ["a", "x" * 256]):
        with pytest.raises(api.UrmapxError) as e:
            api.bam_depth_host(b"", 2, names, [5, 5])
        assert e.value.code == api.E_ARG
    api.bam_depth_host(b"", 2, ["a", "x" * 255], [5, 5])
    for bad in (tiny(0, 5)[:-1], tiny(2, 5), tiny(0, -2)):  # the chain is the sort's: URMAPX_E_FORMAT
        with pytest.raises(api.UrmapxError) as e:
            api.bam_depth_host(bad, 2, ["a", "b"], [50, 50])
        assert e.value.code == -2


def test_structs_in_step_with_the_header():
    assert C.sizeof(api.DepthOpts) == 4 and C.sizeof(api.DepthSummary) == 32
    assert [n for n, _ in api.DepthResult._fields_] == ["text", "text_bytes", "runs", "refs", "n_ref", "text_slices", "records", "stage_chunks", "least_budget",
                                                        "alloc_s", "count_s", "scan_s", "runs_s", "format_s", "copy_s"]
    assert C.sizeof(api.DepthResult) == 112 and api.DepthResult.alloc_s.offset == 64
    header = open(os.path.join(ROOT, "include", "urmapx.h")).read()
    body = header[header.index("typedef struct urmapx_depth_result"):header.index("} urmapx_depth_result;")]
    at = [body.index(w) for w in ("*text;", "text_bytes;", "runs;", "*refs;", " n_ref;", "text_slices;", "records;", "stage_chunks;", "least_budget;", "alloc_s,")]
    assert at == sorted(at)
    assert "Depth (per-base coverage" in header


def test_the_memory_sum_is_monotone_and_counts_the_counters():
    f = api.bam_depth_device_bytes
    base = f(10 ** 6, 10, 1000)
    assert f(10 ** 6 + 1, 10, 1000) > base and f(10 ** 6, 11, 1000) > base and f(10 ** 6, 10, 1001) > base
    for cols, refs, recs in ((0, 0, 0), (1, 1, 1), (3 * 10 ** 9, 3366, 10 ** 9)):
        assert f(cols, refs, recs) >= 4 * (cols + refs) + 8 * recs
        assert f(cols, refs, recs) - api.bam_depth_resident_bytes(cols, refs) >= 8 * recs
    # at a genome's scale the counters are nearly all of it
    assert api.bam_depth_resident_bytes(3 * 10 ** 9, 3366) < 4 * 3 * 10 ** 9 + (128 << 20)


def duplicated_input():
    """pairs and fragments of which more than a quarter are duplicates, some records the marking does not look at, in no order"""
    recs = []
    for k in range(12):
        at = 100 + 37 * (k % 4)  # four places: three pairs at each, two of them duplicates
        recs += pair(b"p%d" % k, (0, at, 0), (0, at + 150, 1), qa=Q(30 + k), qb=Q(30))
    recs += [R(1, 40, 0, "20M", Q(20 + k), b"f%d" % k) for k in range(6)]                   # six fragments at one end: five duplicates
    recs += [R(1, 300, 0x400, "20M", Q(30), b"x"), R(1, 500, 0x100, "20M", Q(30), b"s")]  # an incoming 0x400 on a lone read is cleared
    recs += [R(2, 5, 0x800 | 0x400, "9M", Q(30), b"u"), tiny(-1, -1)]                       # supplementary and flagged: stays flagged
    return b"".join(recs), ["r0", "r1", "r2"], [1000, 800, 30]


def test_the_host_twin_counts_the_flags_as_written():
    """urmapx_bam_sort_with_host with the depth under marking = urmapx_bam_depth_host of the inflated sorted, marked stream; the BAM bytes and the
    index are those of the call without depth"""
    records, names, lens = duplicated_input()
    members, bai, depth, rep = api.bam_sort_host(records, 3, markdup=True, depth=(names, lens), report=True)
    plain = api.bam_sort_host(records, 3, markdup=True)
    assert (members, bai) == plain
    stream = bl.inflate(members)
    flags = ml.flags_of(stream)
    assert sum(1 for f in flags if f & 0x400) * 4 >= len(flags)
    agree(depth, api.bam_depth_host(stream, 3, names, lens))
    agree(depth, dl.model(stream, names, lens))
    assert depth != api.bam_depth_host(records, 3, names, lens)[:3]  # (the incoming flags give another answer)
    assert rep["depth_records"] == len(flags) and rep["records"] == len(flags)
    # without marking the flags are the incoming ones
    _, _, depth0 = api.bam_sort_host(records, 3, depth=(names, lens), depth_mapq=0)
    agree(depth0, dl.model(records, names, lens))


def test_option_and_report_structs_in_step_with_the_header():
    """the options as urmapx_map_files reads them: the fields up to sort_mem where they were, depth_out and depth_mapq appended; the
    report's depth fields behind sort_partitions"""
    full, old = api.MapOptionsDepth, api.MapOptionsSortMem
    assert full._fields_[:-2] == old._fields_ and [n for n, _ in full._fields_[-2:]] == ["depth_out", "depth_mapq"]
    assert all(getattr(full, n).offset == getattr(old, n).offset for n, _ in old._fields_)
    assert full.depth_out.offset == C.sizeof(old) == 88 and full.depth_mapq.offset == 96 and C.sizeof(full) == 104
    rep, before = api.MapReportDepth, api.MapReportSort
    assert rep._fields_[:-4] == before._fields_ and [n for n, _ in rep._fields_[-4:]] == ["depth_s", "depth_runs", "depth_covered", "depth_bases"]
    assert rep.depth_s.offset == C.sizeof(before) and C.sizeof(rep) == C.sizeof(before) + 32
    header = open(os.path.join(ROOT, "include", "urmapx.h")).read()
    opts = header[header.index("typedef struct urmapx_map_options"):header.index("} urmapx_map_options;")]
    assert opts.rindex("uint32_t depth_mapq;") > opts.rindex("const char *depth_out;") > opts.rindex("uint64_t sort_mem;")
    body = header[header.index("typedef struct urmapx_map_report"):header.index("} urmapx_map_report;")]
    assert body.rindex("depth_runs, depth_covered, depth_bases;") > body.rindex("double depth_s;") > body.rindex("uint32_t sort_partitions;")


# ---- urmapx_map_files with depth_out: the stand-alone sanitizer program ----
STUB_MAPS = {"URX_STUB_MAP": "1"}  # the stand-in lanes place every read (a pure function of its bases)


def records_and_refs(path):
    """the records of a BAM file, its references' names and lengths"""
    inflated = bl.inflate(open(path, "rb").read())
    text, refs, _ = bl.read_bam(inflated)
    return inflated[len(bl.bam_header(text, refs)):], [n for n, _ in refs], [l for _, l in refs]


@pytest.mark.parametrize("extra,min_mapq", [([], 0), (["-batch", "64", "-streams", "3"], 0), (["-depthq", "30"], 30)])
def test_pipeline_depth_under_asan(tmp_path, san, extra, min_mapq):  # noqa: F811
    """-sort -markdup -depth through the pipeline: the file is the model's for the records the BAM file holds -- duplicates left out --,
    the BAM file and its index are those of the run without -depth, the totals and the table are the summaries"""
    fq = tmp_path / "in.fq"
    fq.write_bytes(with_copies(open(os.path.join(GOLD, "se150.fq"), "rb").read()))
    plain, out, bed = tmp_path / "p.bam", tmp_path / "d.bam", tmp_path / "d.bedgraph"
    common = ["map", fq, "-biglen", "300000", "-bam", "-sort", "-markdup"]
    assert san_run(san["asan"], common + ["-o", plain], env=STUB_MAPS)[0] == 0
    rc, text = san_run(san["asan"], common + ["-o", out, "-depth", bed] + extra, env=STUB_MAPS)
    assert rc == 0, text
    assert out.read_bytes() == plain.read_bytes() and (tmp_path / "d.bam.bai").read_bytes() == (tmp_path / "p.bam.bai").read_bytes()
    records, names, lens = records_and_refs(out)
    flags = ml.flags_of(records)
    assert sum(1 for f in flags if f & 0x400) >= 10
    want_text, runs, summ = dl.model(records, names, lens, min_mapq)
    assert bed.read_bytes() == want_text
    dl.check_tiling(want_text, names, lens)
    assert "depth runs=%d covered=%d bases=%d\n" % (runs, sum(s["covered"] for s in summ), sum(s["bases"] for s in summ)) in text
    assert sum(s["reads"] for s in summ) > 100 or min_mapq
    for name, l, s in zip(names, lens, summ):
        line = "%s\t%d\t%d\t%d\t%.2f\t%.2f\t%.2f\n" % (name, l, s["reads"], s["covered"], 100.0 * s["covered"] / l, s["bases"] / l,
                                                        s["mapq_sum"] / s["reads"] if s["reads"] else 0.0)
        assert line in text, (line, text)
    if min_mapq == 0:  # the duplicates are left out: the incoming flags would count them
        assert dl.model(ml.mask_dup(records), names, lens)[0] != want_text


def test_refusals_of_the_options(tmp_path, san):  # noqa: F811
    fq = os.path.join(GOLD, "se150.fq")
    out, bed = tmp_path / "no.bam", tmp_path / "no.bedgraph"
    for args, word in ((["-bam", "-depth", bed], "depth_out needs bam_sort"), (["-bam", "-sort", "-depthq", "5"], "depth_mapq needs depth_out"),
                       (["-bam", "-sort", "-depth", bed, "-depthq", "256"], "0 .. 255"),
                       (["-bam", "-sort", "-depth", out], "file of its own"), (["-bam", "-sort", "-depth", str(out) + ".bai"], "file of its own")):
        rc, text = san_run(san["asan"], ["map", fq, "-o", out] + args)
        assert rc == 1 and "rc=-5" in text and word in text, text
        assert not out.exists() and not bed.exists() and not (tmp_path / "no.bam.bai").exists()
    # a budget that does not hold the counters: the least budget is named and nothing is left behind
    rc, text = san_run(san["asan"], ["map", fq, "-o", out, "-biglen", "300000", "-bam", "-sort", "-depth", bed, "-sortmem", "1000000"], env=STUB_MAPS)
    assert rc == 1 and "rc=-3" in text and "at least" in text and "sort_mem" in text, text
    least = int(text.split("at least ")[1].split()[0])
    assert least > 4 * 1550000 and not out.exists() and not bed.exists() and not (tmp_path / "no.bam.bai").exists()


def test_refusals_of_the_command_line(tmp_path):
    """before the index is read (the .ufi named here does not exist), each by the word that is wrong"""
    exe = os.path.join(ROOT, "urmap_amd", "urmap")
    fq, out, bed = os.path.join(GOLD, "se150.fq"), str(tmp_path / "o.bam"), str(tmp_path / "o.bedgraph")
    fifo = str(tmp_path / "pipe")
    os.mkfifo(fifo)
    assert stat.S_ISFIFO(os.stat(fifo).st_mode)
    base = [exe, "-map", fq, "-ufi", str(tmp_path / "none.ufi"), "-bamout", out]
    for args, word in ((["-depth", bed], "-depth needs -sort"), (["-sort", "-depth_mapq", "3"], "-depth_mapq needs -depth"),
                       (["-sort", "-depth", out], "a file of its own"), (["-sort", "-depth", out + ".bai"], "a file of its own"),
                       (["-sort", "-depth", fifo], "not a pipe"), (["-sort", "-depth", "/dev/stdout"], "not a pipe"),
                       (["-sort", "-depth", bed, "-depth_mapq", "256"], "from 0 to 255"), (["-sort", "-depth", bed, "-depth_mapq", "x"], "from 0 to 255")):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and word in r.stderr and "none.ufi" not in r.stderr, (args, r.stderr)
        assert not os.path.exists(out) and not os.path.exists(bed)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)  # (no command: the help text)
    assert "-depth FILE" in r.stdout + r.stderr and "-depth_mapq N" in r.stdout + r.stderr
