"""CPU: the statistics' rule (include/urmapx.h "Stats").  urmapx_bam_stats_host against the model of tests/stats_lib.py on hand-made
records at every edge the rule names, the quotient and the median, the struct layouts and the memory sum, the host twin of the sort
with statistics, and the refusals of the command line."""
import ctypes as C
import os
import stat
import subprocess

import numpy as np
import pytest

import bam_lib as bl
import markdup_lib as ml
import stats_lib as st
from urmap_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES, LENS = ["chrA", "empty", "chrLast"], [5000, 0, 70000]
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1030]
rec = st.rec


def host_equals_model(records, names=NAMES, lens=LENS, command=None):
    got = api.bam_stats_host(records, len(lens), names, lens, command=command)
    want = st.model(records, names, lens, command or b"")
    assert got == want, first_difference(got, want)
    return st.parse(got)


def first_difference(got, want):
    a, b = got.split(b"\n"), want.split(b"\n")
    for k, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return k, x[:200], y[:200]
    return len(a), len(b)


# ---- the inputs, shared with tests/test_gpu_stats.py ----
def length_cases():
    """reads of every length in LENGTHS on both strands, as first and as last fragments, mapped, with random bases and qualities"""
    rng = np.random.default_rng(1)
    recs = []
    for l in LENGTHS:
        for flag in (0, 0x10, 0x81, 0x91):
            seq = rng.choice([1, 2, 4, 8, 15], l)
            recs.append(rec(flag=flag, ref=0, pos=7, mapq=int(rng.integers(0, 61)), cigar="%dM" % l if l else "", seq=seq, qual=bytes(rng.integers(0, 45, l).astype(np.uint8))))
    return b"".join(recs)


def quality_cases():
    """QUAL bytes 0, 93, 94 and 254 at known cycles, a read without qualities, one whose 0xFF is not its first byte"""
    recs = [rec(ref=0, seq=[1] * 6, qual=bytes([0, 93, 94, 254, 255, 40])), rec(flag=0x80, ref=2, seq=[2] * 5, qual=bytes([255] * 5)),
            rec(flag=0x10, ref=0, seq=[4] * 4, qual=bytes([94, 0, 1, 2])), rec(flag=4, seq=[8] * 3, qual=bytes([255, 3, 3]))]
    return b"".join(recs)


def code_cases():
    return b"".join(rec(flag=f, ref=0, seq=list(range(16)) + [3], qual=bytes(range(17))) for f in (0, 0x10, 0x80, 0x90))


TLENS = [-1, 0, 1, 7999, 8000, 8001, 2 ** 31 - 1, -2 ** 31]


def insert_cases():
    recs = []
    for tlen in TLENS:
        for strands in (0, 0x10, 0x20, 0x30):
            recs.append(rec(flag=0x1 | strands, ref=2, next_ref=2, tlen=tlen, seq=[1, 2]))
            recs.append(rec(flag=0x1 | strands, ref=2, next_ref=0, tlen=tlen, seq=[1, 2]))   # the mate elsewhere
    recs += [rec(flag=0x9, ref=2, next_ref=2, tlen=300, seq=[1]), rec(flag=0x5, ref=2, next_ref=2, tlen=300, seq=[1]),  # mate unmapped; unmapped
             rec(flag=0x0, ref=2, next_ref=2, tlen=300, seq=[1])]                                                       # not paired
    return b"".join(recs)


def flag_cases():
    recs = [rec(flag=1 << b, ref=0, mapq=b, cigar="3M1I", seq=[1, 2, 4, 8], aux=b"NMC\x02") for b in range(16)]
    recs += [rec(flag=0x900, ref=0, seq=[1]), rec(flag=0x3, ref=0, seq=[1]), rec(flag=0x7, ref=0, seq=[1])]
    return b"".join(recs)


def cigar_cases():
    every_op = [(k % 3, op) for k, op in enumerate(list(range(16)) * 2)]  # every op code, the unused ones too, lengths 0, 1, 2
    recs = [rec(ref=0, seq=[1] * 4), rec(ref=0, cigar=every_op, seq=[1] * 9), rec(flag=4, ref=0, cigar="5M2I3D", seq=[1] * 7),
            rec(ref=2, cigar=[(l, op) for l in (255, 256, 257, 2 ** 28 - 1, 1, 63, 64) for op in (1, 2)], seq=[2]),
            rec(ref=2, cigar=[(1 + k % 3, (0, 1, 2, 4)[k % 4]) for k in range(65535)], seq=[4] * 3, aux=b"NMi\x07\0\0\0")]
    return b"".join(recs)


def long_cigar_cases(counts=(8, 9, 64, 65, 65535)):
    """CIGARs whose indels lie at both sides of every edge of the sharing: ops LANE_OPS - 1 and LANE_OPS, 63 and 64"""
    recs = []
    for n in counts:
        ops = [(1 + k % 70, (1, 2, 0, 4)[k % 4]) for k in range(n)]
        recs += [rec(ref=0, cigar="4M", seq=[1] * 4), rec(ref=2, cigar=ops, seq=[2, 4], aux=b"XAZab\0NMs\x05\0"), rec(flag=0x10, ref=0, cigar="1I1D", seq=[8])]
    return b"".join(recs)


def aux_cases():
    nm = [b"NMc\xfb", b"NMc\x05", b"NMC\xfb", b"NMs\xff\xff", b"NMs\x2c\x01", b"NMS\xff\xff", b"NMi\xff\xff\xff\xff", b"NMi\x40\x42\x0f\0", b"NMI\xff\xff\xff\xff"]
    front = [b"XZZhello\0", b"XHH1AE3\0", b"XZZ\0"] + [b"XBB" + t + b"\x03\0\0\0" + b"\x01" * (3 * w) for t, w in ((b"c", 1), (b"C", 1), (b"s", 2), (b"S", 2), (b"i", 4), (b"I", 4), (b"f", 4))]
    front += [b"XAAq", b"XFf\0\0\x80\x3f", b"XZZ" + b"y" * 200 + b"\0", b"NMA7", b"NMZ12\0", b"NMf\0\0\0\0"]  # (an NM of another type is walked over)
    cut = [b"NM", b"NMi\x01\0", b"XZZabc", b"XBBi\x03\0\0\0\x01\x01", b"XBB", b"XBBi\xff\xff\xff\xff", b"XAA", b"N", b"XZZ" + b"y" * 64]
    unknown = [b"XQQ1NMC\x01", b"XBBA\x01\0\0\0aNMC\x01", b"XBBZ\0\0\0\0NMC\x01", b"XZ\0\0NMC\x01"]
    recs = [rec(ref=0, cigar="3M1I2D1X1=", seq=[1] * 6, aux=a) for a in nm + [f + b"NMC\x09" for f in front] + cut + unknown + [b"", b"NMC\x03NMC\x05"]]
    recs += [rec(flag=4, ref=0, seq=[1], aux=b"NMC\x09"), rec(ref=0, cigar="2M", seq=[1, 1], aux=b"NMC\x04", l_seq=900)]  # unmapped; SEQ leaves the block
    return b"".join(recs)


def reference_cases():
    return b"".join([rec(flag=4, seq=[1, 2]), rec(ref=2, pos=69999, seq=[2]), rec(flag=0x400, ref=2, seq=[4] * 3), rec(flag=0x404, seq=[]),
                     rec(flag=4, ref=0, seq=[15]), rec(ref=0, mapq=255, seq=[8])])


ALL_CASES = {"lengths": length_cases, "qualities": quality_cases, "codes": code_cases, "inserts": insert_cases, "flags": flag_cases, "cigars": cigar_cases,
             "long cigars": long_cigar_cases, "aux": aux_cases, "references": reference_cases}


# ---- the host twin against the model ----
def test_no_records_at_all():
    t = host_equals_model(b"")
    assert t["#"] == ["# urmapx stats 1", "# command: "] and t["SN"]["records"] == "0" and t["SN"]["error rate"] == "0.000000"
    assert t["SN"]["average length"] == "0.00" and t["SN"]["insert size median"] == "0"
    assert t["RF"] == [("chrA", 5000, 0, 0, 0), ("empty", 0, 0, 0, 0), ("chrLast", 70000, 0, 0, 0), ("*", 0, 0, 0, 0)]
    assert not any(t[s] for s in ("RL", "MQ", "IS", "FFQ", "LFQ", "BC", "GC", "ID"))
    assert api.bam_stats_host(b"", 0, [], []).endswith(b"SN\tinsert size median\t0\nRF\t*\t0\t0\t0\t0\n")
    assert host_equals_model(b"", command=b"urmap -map x -stats y")["#"][1] == "# command: urmap -map x -stats y"


def test_lengths_at_the_caps_on_both_strands():
    t = host_equals_model(length_cases())
    assert sorted(t["RL"]) == LENGTHS and all(v == (2, 2) for v in t["RL"].values())
    assert t["SN"]["maximum length"] == "1030" and t["SN"]["reads"] == str(4 * len(LENGTHS))
    for table in ("FFQ", "LFQ", "BC"):
        assert list(t[table])[:3] == [1, 2, 3] and list(t[table])[-2:] == [1024, ">1024"] and len(t[table]) == 1025
        width = 6 if table == "BC" else 94
        assert all(len(v) == width for v in t[table].values())
        per_class = 2 if table != "BC" else 4
        assert sum(t[table][">1024"]) == per_class * (1 + 6) and sum(t[table][1024]) == per_class * 3 and sum(t[table][1]) == per_class * 13


def test_a_reversed_read_is_read_from_its_end_and_complemented():
    fwd = host_equals_model(rec(ref=0, seq=[1, 1, 2, 8], qual=bytes([10, 11, 12, 13])))
    rev = host_equals_model(rec(flag=0x10, ref=0, seq=[1, 1, 2, 8], qual=bytes([10, 11, 12, 13])))
    assert [fwd["BC"][c] for c in (1, 2, 3, 4)] == [(1, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0), (0, 0, 0, 1, 0, 0)]
    assert [rev["BC"][c] for c in (1, 2, 3, 4)] == [(1, 0, 0, 0, 0, 0), (0, 0, 1, 0, 0, 0), (0, 0, 0, 1, 0, 0), (0, 0, 0, 1, 0, 0)]
    assert [v.index(1) for v in fwd["FFQ"].values()] == [10, 11, 12, 13] and [v.index(1) for v in rev["FFQ"].values()] == [13, 12, 11, 10]
    assert fwd["GC"] == rev["GC"] == {25: 1}


def test_quality_bytes_at_the_cap_and_reads_without_qualities():
    t = host_equals_model(quality_cases())
    assert t["SN"]["reads without qualities"] == "2" and t["SN"]["average quality"] == st.quotient(0 + 93 * 4 + 40 + 93 + 0 + 1 + 2, 10, 2)
    assert t["FFQ"][2][93] == t["FFQ"][3][93] == t["FFQ"][5][93] == 1 and t["FFQ"][1][0] == 1 and "LFQ" in t and not t["LFQ"]
    assert sum(sum(v) for v in t["BC"].values()) == 18


def test_every_base_code():
    t = host_equals_model(code_cases())
    assert t["BC"][1] == (0, 0, 0, 0, 0, 4) and t["BC"][2] == (2, 0, 0, 0, 2, 0) and t["BC"][16] == (0, 0, 0, 2, 2, 0) and t["GC"] == {11: 4}
    # (cycle 2 of a reversed read is its base 15, an N; its cycle 16 is base 1, an A read as T)


def test_insert_sizes_at_the_cap_by_orientation():
    t = host_equals_model(insert_cases())
    assert t["IS"] == {1: (4, 1, 1, 2), 7999: (4, 1, 1, 2), 8000: (12, 3, 3, 6)}
    assert t["SN"]["pairs with insert size"] == "20" and t["SN"]["inward pairs"] == "5" and t["SN"]["other pairs"] == "10"
    assert t["SN"]["mate on another reference"] == str(4 * len(TLENS)) and t["SN"]["insert size median"] == "8000"
    assert t["SN"]["insert size average"] == st.quotient(4 + 4 * 7999 + 12 * 8000, 20, 2)


def test_every_flag_bit_alone():
    t = host_equals_model(flag_cases())
    sn = {k: int(v) for k, v in t["SN"].items() if "." not in v}
    assert sn["records"] == 19 and sn["secondary"] == 2 and sn["supplementary"] == 2 and sn["reads"] == 16
    assert sn["reads paired"] == 3 and sn["reads unmapped"] == 2 and sn["last fragments"] == 1 and sn["reads properly paired"] == 1
    assert sn["reads duplicated"] == 1 and sn["reads QC failed"] == 1 and sn["reads reverse strand"] == 1 and sn["singletons"] == 0
    assert sn["reads MQ0"] == 2 and sn["reads with NM"] == 13 and sn["mismatches"] == 26 and sn["insertions"] == 13 and sn["bases duplicated"] == 4


def test_cigars_of_every_op_and_length():
    t = host_equals_model(cigar_cases())
    assert t["ID"][255] == (1, 1) and t["ID"][256] == (3, 3) and 257 not in t["ID"] and 0 not in t["ID"]
    assert int(t["SN"]["insertions"]) == 2 + 7 + 16384 and int(t["SN"]["deletions"]) == 1 + 7 + 16384
    assert t["SN"]["reads with NM"] == "1" and t["SN"]["mismatches"] == "7"


def test_long_cigars():
    host_equals_model(long_cigar_cases())


def test_nm_in_every_type_and_behind_every_other_field():
    t = host_equals_model(aux_cases())
    assert int(t["SN"]["reads with NM"]) == 9 + 16 + 1 and int(t["SN"]["mismatches"]) == 5 + 251 + 300 + 65535 + 1000000 + (2 ** 32 - 1) + 9 * 16 + 3
    assert t["SN"]["error rate"] == st.quotient(int(t["SN"]["mismatches"]), 6 * 26, 6)


def test_no_reference_the_last_reference_and_an_empty_one():
    t = host_equals_model(reference_cases())
    assert t["RF"] == [("chrA", 5000, 1, 1, 0), ("empty", 0, 0, 0, 0), ("chrLast", 70000, 2, 0, 1), ("*", 0, 0, 2, 1)]
    assert t["MQ"] == {0: 2, 255: 1} and t["SN"]["reads MQ0"] == "2" and t["GC"] == {0: 2, 50: 1, 100: 2}


@pytest.mark.parametrize("case", list(ALL_CASES))
def test_cases_one_after_the_other_in_one_input(case):
    """each input behind all the others: the counters add up"""
    both = ALL_CASES[case]() + b"".join(f() for k, f in ALL_CASES.items() if k not in (case, "cigars", "long cigars"))
    host_equals_model(both)


def test_quotients_at_exact_halves_and_without_a_denominator():
    assert [st.quotient(*a) for a in ((1, 8, 2), (3, 8, 2), (5, 1000, 2), (15, 1000, 2), (0, 0, 2), (7, 0, 6), (2, 3, 6))] == \
        ["0.13", "0.38", "0.01", "0.02", "0.00", "0.000000", "0.666667"]
    # total length 1 over 8 reads: 0.125 -> 0.13; 3 over 8: 0.375 -> 0.38; no read at all: 0.00
    for total, want in ((1, "0.13"), (3, "0.38")):
        recs = b"".join(rec(flag=4, seq=[1] * (1 if k < total else 0)) for k in range(8))
        assert host_equals_model(recs)["SN"]["average length"] == want
    # mismatches 1 over 2 000 000 aligned bases: 0.0000005 -> 0.000001
    t = host_equals_model(rec(ref=0, cigar="2000000M", seq=[1], aux=b"NMC\x01"))
    assert t["SN"]["error rate"] == "0.000001" and t["SN"]["average quality"] == "30.00"
    assert host_equals_model(rec(ref=0, cigar="5S", seq=[1], aux=b"NMC\x01"))["SN"]["error rate"] == "0.000000"


@pytest.mark.parametrize("sizes,median,average", [((), "0", "0.00"), ((300,), "300", "300.00"), ((300, 401), "300", "350.50"), ((9000, 8000, 70000), "8000", "8000.00"),
                                                  ((5, 6, 7, 8), "6", "6.50"), ((5, 6, 7), "6", "6.00")])
def test_the_median_of_the_insert_sizes(sizes, median, average):
    t = host_equals_model(b"".join(rec(flag=0x21, ref=0, next_ref=0, tlen=s, seq=[1]) for s in sizes))
    assert t["SN"]["insert size median"] == median and t["SN"]["insert size average"] == average and t["SN"]["pairs with insert size"] == str(len(sizes))


def test_refusals_of_the_arguments():
    for names in (["a", ""], ["a", "x" * 256]):
        with pytest.raises(api.UrmapxError) as e:
            api.bam_stats_host(b"", 2, names, [5, 5])
        assert e.value.code == api.E_ARG
    for bad in (rec(ref=0)[:-1], rec(ref=2), rec(ref=0, pos=-2)):  # the chain is the sort's: URMAPX_E_FORMAT
        with pytest.raises(api.UrmapxError) as e:
            api.bam_stats_host(bad, 2, ["a", "b"], [50, 50])
        assert e.value.code == -2


def test_structs_and_the_memory_sum_in_step_with_the_header():
    assert [n for n, _ in api.StatsResult._fields_] == ["text", "text_bytes", "records", "reads", "mapped", "properly_paired", "duplicated", "insert_median",
                                                        "stage_chunks", "least_budget", "alloc_s", "count_s", "format_s"]
    assert C.sizeof(api.StatsResult) == 104 and api.StatsResult.alloc_s.offset == 80
    # the one struct of what the planned sort takes on the way: twelve fields, the statistics' command at 48, the pileup's from 56 on
    assert [n for n, _ in api.BamSortExtras._fields_] == ["md", "dopts", "names", "lens", "depth", "stats", "stats_command", "popts", "seqs", "index", "pileup",
                                                          "pileup_command"]
    assert C.sizeof(api.BamSortExtras) == 96 and api.BamSortExtras.stats_command.offset == 48 and api.BamSortExtras.popts.offset == 56
    header = open(os.path.join(ROOT, "include", "urmapx.h")).read()
    body = header[header.index("typedef struct urmapx_stats_result"):header.index("} urmapx_stats_result;")]
    at = [body.index(w) for w in ("*text;", "text_bytes;", "records,", " reads,", "insert_median;", "stage_chunks;", "least_budget;", "alloc_s,")]
    assert at == sorted(at) and "Stats (alignment QC tables" in header
    body = header[header.index("typedef struct urmapx_bam_sort_extras {"):header.index("} urmapx_bam_sort_extras;")]
    at = [body.index(w) for w in ("*md;", "*dopts;", "*names;", "*lens;", "*depth;", "*stats;", "*stats_command;", "*popts;", "*seqs;", "*index;", "*pileup;",
                                  "*pileup_command;")]
    assert at == sorted(at) and body.count(";") == 12
    # the tables: 64 SN words, MQ, GC, ID, IS, RL, BC, both quality tables, three words a reference and three more
    words = 64 + 256 + 104 + 2 * 257 + 3 * 8001 + 2 * 65536 + 6 * 1025 + 2 * 94 * 1025
    assert api.bam_stats_resident_bytes(0) == 8 * (words + 3) + 4096 and api.bam_stats_resident_bytes(1000) - api.bam_stats_resident_bytes(0) == 24000
    assert api.bam_stats_resident_bytes(3366) < 4 << 20


# ---- the host sort with statistics ----
def test_the_host_twin_of_the_sort_counts_the_flags_as_written():
    from test_depth_cpu import duplicated_input
    records, names, lens = duplicated_input()
    members, bai, text, rep = api.bam_sort_host(records, 3, markdup=True, stats=(names, lens), report=True)
    assert (members, bai) == api.bam_sort_host(records, 3, markdup=True)
    stream = bl.inflate(members)
    assert text == st.model(stream, names, lens) == api.bam_stats_host(stream, 3, names, lens)
    t = st.parse(text)
    flagged = 2 * rep["pairs_duplicate"] + rep["fragments_duplicate"]
    assert int(t["SN"]["reads duplicated"]) == flagged == rep["stats_duplicated"] > 10
    assert sum(1 for f in ml.flags_of(stream) if f & 0x400 and not f & 0x900) == flagged
    assert text != st.model(records, names, lens)  # (the incoming flags give another answer)
    assert rep["stats_records"] == len(ml.flags_of(stream)) == int(t["SN"]["records"])
    # with the depth beside it: both as they are alone; without marking the flags are the incoming ones
    members2, bai2, depth, text2 = api.bam_sort_host(records, 3, markdup=True, depth=(names, lens), stats=(names, lens))
    assert (members2, bai2, text2) == (members, bai, text) and depth == api.bam_sort_host(records, 3, markdup=True, depth=(names, lens))[2]
    assert api.bam_sort_host(records, 3, stats=(names, lens))[2] == st.model(records, names, lens)


# ---- the command line ----
def test_refusals_of_the_command_line(tmp_path):
    """before the index is read (the .ufi named here does not exist), each by the word that is wrong"""
    exe = os.path.join(ROOT, "urmap_amd", "urmap")
    fq, out, txt = os.path.join(GOLD, "se150.fq"), str(tmp_path / "o.bam"), str(tmp_path / "o.stats")
    fifo = str(tmp_path / "pipe")
    os.mkfifo(fifo)
    assert stat.S_ISFIFO(os.stat(fifo).st_mode)
    base = [exe, "-map", fq, "-ufi", str(tmp_path / "none.ufi"), "-bamout", out]
    for args, word in ((["-stats", txt], "-stats needs -sort"), (["-sort", "-stats", ""], "-stats needs a file name"),
                       (["-sort", "-stats", out], "a file of their own"), (["-sort", "-stats", out + ".bai"], "a file of their own"),
                       (["-sort", "-depth", txt, "-stats", txt], "a file of their own"),
                       (["-sort", "-stats", fifo], "not a pipe"), (["-sort", "-stats", "/dev/stdout"], "not a pipe")):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and word in r.stderr and "-stats" in r.stderr and "none.ufi" not in r.stderr, (args, r.stderr)
        assert not os.path.exists(out) and not os.path.exists(txt)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)  # (no command: the help text)
    assert "-stats FILE" in r.stdout + r.stderr
