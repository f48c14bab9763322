"""CPU: the pileup's rule (include/urmapx.h "Pileup").  urmapx_bam_pileup_host against the model of tests/pileup_lib.py, byte for byte,
on hand-made records at every edge the rule names; the struct layouts and the memory sum; the refusals of the arguments and of the
command line; the host twin of the sort with the pileup, alone and beside marking, depth and statistics."""
import ctypes as C
import os
import stat
import subprocess

import numpy as np
import pytest

import bam_lib as bl
import depth_lib as dl
import markdup_lib as ml
import pileup_lib as pl
from stats_lib import rec
from test_stats_cpu import first_difference, long_cigar_cases
from urmap_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CODE = {"A": 1, "C": 2, "G": 4, "T": 8}
ANY = {"min_alt": 1, "min_pct": 0}       # every base that differs is an allele


def reference():
    """four references: lower case at chrA 100 .. 109, N and IUPAC letters at 200 .. 209, an empty one, chrA ending in A where chrB
    begins with C, chrB in lower case throughout"""
    rng = np.random.default_rng(5)
    names, lens = ["chrA", "empty", "chrB", "chrLast"], [5000, 0, 300, 70000]
    seqs = [bytearray(rng.choice(list(b"ACGT"), l).astype(np.uint8).tobytes()) for l in lens]
    seqs[0][100:110] = bytes(seqs[0][100:110]).lower()
    seqs[0][200:210] = b"NNNNNRYKMn"
    seqs[0][-1:] = b"A"
    seqs[2] = bytearray(bytes(seqs[2]).lower())
    seqs[2][:1] = b"c"
    return names, lens, [bytes(s) for s in seqs]


NAMES, LENS, SEQS = reference()


def matching(ref, pos, n):
    """the 4-bit codes of n reference bases from pos on (15 for a letter that is none of ACGT, 1 beyond the end)"""
    s = SEQS[ref][pos:pos + n].upper().decode()
    return [CODE.get(ch, 15) for ch in s] + [1] * (n - len(s))


def other(codes, by=1):
    """every base replaced by the one `by` places on in A C G T"""
    return [(1, 2, 4, 8)[((1, 2, 4, 8).index(c) + by) % 4] if c in (1, 2, 4, 8) else c for c in codes]


def host_equals_model(records, opts=None, names=NAMES, lens=LENS, seqs=SEQS, command=None):
    got = api.bam_pileup_host(records, len(lens), names, lens, seqs, opts=opts, command=command)
    want = pl.model(records, names, lens, seqs, opts, command or b"")
    assert got == want, first_difference(got, want)
    return pl.parse(got)


# ---- the inputs, shared with tests/test_gpu_pileup.py ----
def lane_cases():
    """M runs of every length at the edges of 64 lanes behind soft clips of 0, 1 and 3 bases (both nibble parities at the run's start),
    l_seq odd and even, read names of 1 .. 8 bytes (records at every byte alignment); every base differs from the reference"""
    recs, k = [], 0
    for run in (1, 63, 64, 65, 127, 128, 129, 150):
        for clip in (0, 1, 3):
            for tail in (0, 1):
                k += 1
                cigar = ("%dS" % clip if clip else "") + "%dM" % run + ("%dS" % tail if tail else "")
                seq = [2] * clip + other(matching(3, 1000 + 7 * k, run), 1 + k % 3) + [4] * tail
                recs.append(rec(ref=3, pos=1000 + 7 * k, mapq=30, cigar=cigar, seq=seq, qual=bytes([13 + (i * 7 + k) % 30 for i in range(len(seq))]), name=b"n" * (1 + k % 8)))
    return b"".join(recs)


def cigar_cases():
    """every op kind (the unused codes too); 63, 64, 65 and 200 ops; 65 535 ops; a CIGAR whose query length exceeds l_seq"""
    rng = np.random.default_rng(9)
    recs = [rec(ref=0, pos=300, cigar=[(3 + k % 4, op) for k, op in enumerate(list(range(16)) * 2)], seq=rng.choice([1, 2, 4, 8], 120))]
    for n in (63, 64, 65, 200, 65535):
        ops = [(1 + k % 3, (0, 1, 7, 2, 8, 4, 3, 0)[k % 8]) for k in range(n)]
        l_seq = sum(l for l, op in ops if op in (0, 1, 4, 7, 8))
        recs.append(rec(ref=3, pos=2000 + n % 100, cigar=ops, seq=rng.choice([1, 2, 4, 8, 15], l_seq), qual=bytes(rng.integers(0, 40, l_seq).astype(np.uint8))))
    recs.append(rec(ref=0, pos=50, cigar="50M", seq=other(matching(0, 50, 30))))                      # the query runs out inside the op
    recs.append(rec(ref=0, pos=3000, cigar="10M5I10M", seq=other(matching(0, 3000, 12))))                 # ... inside an insertion
    recs.append(rec(ref=0, pos=3100, cigar="4M", seq=other(matching(0, 3100, 4)), l_seq=900))                          # SEQ leaves the block: a record, no base
    return b"".join(recs) + long_cigar_cases()


def edge_cases():
    """columns 0 and l_ref - 1; a run past l_ref; pos >= l_ref; the last column of chrA and the first of chrB; the empty reference;
    refID -1"""
    recs = [rec(ref=0, pos=0, cigar="5M", seq=other(matching(0, 0, 5))), rec(ref=0, pos=4995, cigar="5M", seq=other(matching(0, 4995, 5))),
            rec(ref=0, pos=4990, cigar="30M", seq=other(matching(0, 4990, 30))), rec(ref=0, pos=5000, cigar="5M", seq=[1] * 5),
            rec(ref=0, pos=2 ** 31 - 1, cigar="5M", seq=[1] * 5), rec(ref=2, pos=0, cigar="5M", seq=other(matching(2, 0, 5))),
            rec(ref=2, pos=299, cigar="2M", seq=[1, 2]), rec(ref=1, pos=0, cigar="5M", seq=[1] * 5), rec(flag=4, seq=[1] * 5), rec(cigar="5M", seq=[1] * 5),
            rec(ref=3, pos=69999, cigar="1M", seq=other(matching(3, 69999, 1))), rec(ref=3, pos=69990, cigar="5M5D5M", seq=other(matching(3, 69990, 10)))]
    return b"".join(recs)


def filter_cases():
    """each flag of 0x704 alone, 0x800, MAPQ 19 and 20, qualities 12 and 13, no qualities, the codes 0, 3 and 15 (under min_mapq 20)"""
    recs = [rec(flag=f, ref=0, pos=400 + 10 * k, mapq=40, cigar="6M", seq=other(matching(0, 400 + 10 * k, 6))) for k, f in enumerate((0, 0x4, 0x100, 0x200, 0x400, 0x800, 0x10, 0x1))]
    recs += [rec(ref=0, pos=500, mapq=q, cigar="6M", seq=other(matching(0, 500, 6), 2)) for q in (19, 20, 255)]
    recs += [rec(ref=0, pos=600, mapq=30, cigar="6M", seq=other(matching(0, 600, 6)), qual=bytes([12, 13, 12, 13, 0, 255]))]
    recs += [rec(ref=0, pos=700, mapq=30, cigar="6M", seq=other(matching(0, 700, 6)), qual=bytes([255, 0, 0, 0, 0, 0]))]
    recs += [rec(ref=0, pos=800, mapq=30, cigar="6M", seq=[0, 3, 15, 1, 2, 4])]
    return b"".join(recs)


def letter_cases():
    """reads that match the lower-case stretch, reads that differ everywhere over the N and IUPAC columns"""
    recs = [rec(ref=0, pos=95, cigar="20M", seq=matching(0, 95, 20))] * 3
    recs += [rec(ref=0, pos=195, cigar="20M", seq=[(1, 2, 4, 8)[k]] * 20) for k in range(4) for _ in range(3)]
    recs += [rec(ref=2, pos=0, cigar="20M", seq=matching(2, 0, 20))] * 3
    return b"".join(recs)


def pile(column, n_by_code, ref=0):
    """single-base reads on one column: n_by_code[c] of them carry code c"""
    return b"".join(rec(ref=ref, pos=column, cigar="1M", seq=[c]) * n for c, n in n_by_code.items())


def column_with(column, n_ref, alts):
    """n_ref reads of the reference's base and alts[k] reads of the k-th other base"""
    here = matching(0, column, 1)[0]
    return pile(column, dict([(here, n_ref)] + [(other([here], k + 1)[0], n) for k, n in enumerate(alts)]))


# ---- the host twin against the model ----
def test_no_records_at_all():
    t = host_equals_model(b"", command=b"urmap -map x -vcfout y")
    assert t == {"command": "urmap -map x -vcfout y", "contigs": list(zip(NAMES, LENS)), "sites": []}
    assert api.bam_pileup_host(b"", 0, [], [], []).startswith(b"##fileformat=VCFv4.2\n##source=urmap\n##urmapCommand=\n##INFO=<ID=DP")


@pytest.mark.parametrize("opts", [None, ANY, {"min_baseq": 0, "min_alt": 1}], ids=["defaults", "any", "baseq 0"])
def test_lanes_and_nibbles(opts):
    t = host_equals_model(lane_cases(), opts)
    assert len(t["sites"]) > 300


def test_cigars():
    t = host_equals_model(cigar_cases(), ANY)
    cols = {(c, p) for c, p, *_ in t["sites"]}
    assert ("chrA", 51) in cols and ("chrA", 80) in cols and ("chrA", 81) not in cols     # 30 of 50M have bases
    assert ("chrA", 3001) in cols and ("chrA", 3010) in cols and ("chrA", 3011) not in cols  # 10M and two bases of 5I: none left for the second 10M
    assert ("chrA", 3101) not in cols
    host_equals_model(cigar_cases(), {"min_baseq": 20, "min_alt": 2, "min_pct": 30})


def test_reference_edges():
    t = host_equals_model(edge_cases(), ANY)
    cols = [(c, p) for c, p, *_ in t["sites"]]
    assert cols[0] == ("chrA", 1) and ("chrA", 5000) in cols and ("chrB", 1) in cols and cols[-1] == ("chrLast", 70000)
    at = {(c, p): (r, a, dp) for c, p, r, a, dp, _ in t["sites"]}
    assert at["chrA", 5000][0] == "A" and at["chrB", 1][0] == "C" and at["chrA", 5000][2] == 2 and not any(c == "empty" for c, _ in cols)
    assert ("chrLast", 69996) not in cols and ("chrLast", 70001) not in cols


def test_fifteen_hundred_references():
    rng = np.random.default_rng(2)
    names, lens = ["c%d" % k for k in range(1500)], [(k * 7) % 40 for k in range(1500)]
    seqs = [rng.choice(list(b"ACGT"), l).astype(np.uint8).tobytes() for l in lens]
    recs = b"".join(rec(ref=r, pos=0, cigar="50M", seq=rng.choice([1, 2, 4, 8], 50)) for r in range(0, 1500, 3))
    t = host_equals_model(recs, ANY, names, lens, seqs)
    assert len({c for c, *_ in t["sites"]}) > 400 and t["sites"][-1][0] == "c1497"


def test_filters():
    opts = dict(ANY, min_mapq=20)
    t = host_equals_model(filter_cases(), opts)
    at = {p: dp for c, p, r, a, dp, _ in t["sites"]}
    assert [p for p in at if p < 500] == [401 + 10 * k + i for k in (0, 5, 6, 7) for i in range(6)]    # no flag, 0x800, 0x10, 0x1
    assert at[501] == 2 and [p for p in at if 600 <= p < 700] == [602, 604, 606] and [p for p in at if 700 <= p < 800] == list(range(701, 707))
    assert 801 not in at and 802 not in at and 803 not in at
    assert api.bam_pileup_host(filter_cases(), 4, NAMES, LENS, SEQS, opts=opts, report=True)[1]["records"] == 4 + 2 + 3
    host_equals_model(filter_cases())


def test_reference_letters():
    t = host_equals_model(letter_cases(), ANY)
    cols = {(c, p): r for c, p, r, *_ in t["sites"]}
    assert not any(c == "chrA" and (96 <= p <= 115 or 201 <= p <= 210) for c, p in cols) and not any(c == "chrB" for c, _ in cols)
    assert all(("chrA", p) in cols for p in (196, 197, 198, 199, 200, 211, 212))


def test_the_site_rule_at_its_thresholds():
    # min_alt 3: two reads are none, three are one
    t = host_equals_model(column_with(1000, 5, [2]) + column_with(1001, 5, [3]), {"min_pct": 0})
    assert [p for _, p, *_ in t["sites"]] == [1002]
    # 3 of 30 is 10 per cent exactly; 3 of 31 is less
    t = host_equals_model(column_with(1000, 27, [3]) + column_with(1001, 28, [3]))
    assert [(p, dp, ad) for _, p, _, _, dp, ad in t["sites"]] == [(1001, 30, [27, 3])]
    # two and three alleles by count, a tie in the order A C G T, a tie of all three
    t = host_equals_model(column_with(1000, 4, [3, 5]) + column_with(1001, 1, [4, 6, 5]) + column_with(1002, 0, [4, 4]) + column_with(1003, 2, [3, 3, 3]))
    assert [len(a) for _, _, _, a, _, _ in t["sites"]] == [2, 3, 2, 3] and [ad[1:] for *_, ad in t["sites"]] == [[5, 3], [6, 5, 4], [4, 4], [3, 3, 3]]
    for _, _, _, alts, _, ad in t["sites"][2:]:
        assert alts == sorted(alts, key="ACGT".index)
    # min_pct 0 and 100: one read among many; only a column without any other base
    both = column_with(1000, 500, [1]) + column_with(1001, 0, [4]) + column_with(1002, 1, [400])
    assert [p for _, p, *_ in host_equals_model(both, {"min_alt": 1, "min_pct": 0})["sites"]] == [1001, 1002, 1003]
    assert [p for _, p, *_ in host_equals_model(both, {"min_alt": 1, "min_pct": 100})["sites"]] == [1002]
    assert [p for _, p, *_ in host_equals_model(both, {"min_alt": 1, "min_pct": 99})["sites"]] == [1002, 1003]


def test_cases_one_after_the_other_in_one_input():
    host_equals_model(lane_cases() + edge_cases() + filter_cases() + letter_cases() + cigar_cases(), {"min_alt": 2, "min_pct": 5})


def test_dp_is_the_depth_where_every_base_counts():
    """min_baseq 0 and reads without N: a site's DP is the depth of its column for the same MAPQ floor"""
    records = lane_cases() + edge_cases()
    t = host_equals_model(records, {"min_mapq": 10, "min_baseq": 0, "min_alt": 1, "min_pct": 0})
    depth = {}
    for name, beg, end, d in dl.parse(api.bam_depth_host(records, 4, NAMES, LENS, min_mapq=10)[0]):
        depth[name.decode()] = depth.get(name.decode(), []) + [(beg, end, d)]
    assert len(t["sites"]) > 300
    for chrom, pos, _, _, dp, _ in t["sites"]:
        assert [d for b, e, d in depth[chrom] if b <= pos - 1 < e] == [dp]


# ---- the arguments ----
def test_refusals_of_the_arguments():
    for opts in ({"min_mapq": 256}, {"min_baseq": 256}, {"min_alt": 0}, {"min_pct": 101}):
        with pytest.raises(api.UrmapxError) as e:
            api.bam_pileup_host(b"", 4, NAMES, LENS, SEQS, opts=opts)
        assert e.value.code == api.E_ARG
    for names in (["a", ""], ["a", "x" * 256]):
        with pytest.raises(api.UrmapxError) as e:
            api.bam_pileup_host(b"", 2, names, [1, 1], [b"A", b"C"])
        assert e.value.code == api.E_ARG
    for bad in (rec(ref=0)[:-1], rec(ref=4), rec(ref=0, pos=-2)):  # the chain is the sort's: URMAPX_E_FORMAT
        with pytest.raises(api.UrmapxError) as e:
            api.bam_pileup_host(bad, 4, NAMES, LENS, SEQS)
        assert e.value.code == -2
    assert api.bam_pileup_host(b"", 4, NAMES, LENS, SEQS, opts={"min_mapq": 255, "min_baseq": 255, "min_alt": 2 ** 31, "min_pct": 100})


def test_structs_and_the_memory_sum_in_step_with_the_header():
    assert [n for n, _ in api.PileupResult._fields_] == ["text", "text_bytes", "sites", "alt_alleles", "records", "stage_chunks", "least_budget", "alloc_s",
                                                         "count_s", "sites_s", "format_s", "copy_s"]
    assert C.sizeof(api.PileupResult) == 96 and api.PileupResult.alloc_s.offset == 56 and C.sizeof(api.PileupOpts) == 16
    assert [n for n, _ in api.BamSortExtras._fields_] == ["md", "dopts", "names", "lens", "depth", "stats", "stats_command", "popts", "seqs", "index", "pileup",
                                                          "pileup_command"]
    assert C.sizeof(api.BamSortExtras) == 96 and api.BamSortExtras.popts.offset == 56 and api.BamSortExtras.stats_command.offset == 48
    assert C.sizeof(api.MapOptionsPileup) == C.sizeof(api.MapOptionsStats) + 24 and api.MapOptionsPileup.vcf_out.offset == C.sizeof(api.MapOptionsStats)
    assert C.sizeof(api.MapReportPileup) == C.sizeof(api.MapReportStats) + 32 and api.MapReportPileup.pileup_s.offset == C.sizeof(api.MapReportStats)
    header = open(os.path.join(ROOT, "include", "urmapx.h")).read()
    for struct, words in (("urmapx_pileup_result", ("*text;", "text_bytes;", "sites,", "alt_alleles,", "records;", "stage_chunks;", "least_budget;", "alloc_s,", "count_s,",
                                                    "sites_s,", "format_s,", "copy_s;")),
                          ("urmapx_bam_sort_extras", ("*md;", "*dopts;", "*names;", "*lens;", "*depth;", "*stats;", "*stats_command;", "*popts;", "*seqs;", "*index;",
                                                      "*pileup;", "*pileup_command;")),
                          ("urmapx_pileup_opts", ("min_mapq,", "min_baseq,", "min_alt,", "min_pct;"))):
        body = header[header.index("typedef struct " + struct + " {"):header.index("} " + struct + ";")]
        at = [body.index(w) for w in words]
        assert at == sorted(at), struct
    body = header[header.index("typedef struct urmapx_map_options"):header.index("} urmapx_map_options;")]
    at = [body.index(w) for w in ("*stats_out;", "*vcf_out;", "vcf_mapq;", "vcf_baseq;", "vcf_min_alt;", "vcf_min_pct;")]
    assert at == sorted(at) and "---- Pileup (SNV candidate sites" in header
    body = header[header.index("typedef struct urmapx_map_report"):header.index("} urmapx_map_report;")]
    at = [body.index(w) for w in ("stats_s;", "pileup_s;", "pileup_sites;", "pileup_records,")]
    assert at == sorted(at)
    # 16 bytes a column, 16 a reference, a count per 256 columns of a segment, two slices of 2^18 entries of 24 bytes; a byte a base more without a resident store
    cols = 20_000_000
    own = api.bam_pileup_resident_bytes(cols, 3, True)
    assert own == 16 * cols + 16 * 4 + 4 * (16384 + 1) + 2 * 24 * (1 << 18) + (1 << 16)
    assert api.bam_pileup_resident_bytes(cols, 3) == own + cols
    assert api.bam_pileup_resident_bytes(1000, 3, True) == 16 * 1000 + 64 + 4 * 5 + 2 * 24 * (1 << 18) + (1 << 16)
    assert api.bam_pileup_device_bytes(cols, 3, 1000) == own + cols + 8 * 1001 + 2 * ((16 << 20) + 16)
    assert 49e9 < api.bam_pileup_resident_bytes(3_100_000_000, 25, True) < 50e9


# ---- the host sort with the pileup ----
def sort_input():
    from test_depth_cpu import duplicated_input
    records, names, lens = duplicated_input()
    rng = np.random.default_rng(3)
    return records, names, lens, [rng.choice(list(b"ACGT"), l).astype(np.uint8).tobytes() for l in lens]


def test_the_host_twin_of_the_sort_counts_the_flags_as_written():
    records, names, lens, seqs = sort_input()
    members, bai, vcf, rep = api.bam_sort_host(records, 3, markdup=True, pileup=(names, lens, seqs, ANY), report=True)
    assert (members, bai) == api.bam_sort_host(records, 3, markdup=True)
    stream = bl.inflate(members)
    assert vcf == pl.model(stream, names, lens, seqs, ANY) == api.bam_pileup_host(stream, 3, names, lens, seqs, opts=ANY)
    assert vcf != pl.model(records, names, lens, seqs, ANY)  # (the incoming flags give another answer)
    counted = sum(1 for f, r in zip(ml.flags_of(stream), pl.split(stream)) if not f & 0x704 and int.from_bytes(r[4:8], "little", signed=True) >= 0)
    t = pl.parse(vcf)
    assert rep["pileup_records"] == counted and rep["pileup_sites"] == len(t["sites"]) > 100
    assert rep["pileup_alt_alleles"] == sum(len(a) for _, _, _, a, _, _ in t["sites"])
    # at the four places of the pairs one of three pairs is left: no column there is deeper than the pairs that were kept
    assert max(dp for c, p, _, _, dp, _ in t["sites"] if c == "r0") < 12
    # beside the depth and the statistics: each as it is alone; without marking the flags are the incoming ones
    out = api.bam_sort_host(records, 3, markdup=True, depth=(names, lens), stats=(names, lens), pileup=(names, lens, seqs, ANY))
    assert out[:2] == (members, bai) and out[4] == vcf
    assert out[2:4] == api.bam_sort_host(records, 3, markdup=True, depth=(names, lens), stats=(names, lens))[2:4]
    assert api.bam_sort_host(records, 3, pileup=(names, lens, seqs, ANY))[2] == pl.model(records, names, lens, seqs, ANY)
    # the defaults, and a refusal that leaves nothing behind
    assert api.bam_sort_host(records, 3, markdup=True, pileup=(names, lens, seqs, None))[2] == pl.model(stream, names, lens, seqs)
    with pytest.raises(api.UrmapxError) as e:
        api.bam_sort_host(records, 3, markdup=True, pileup=(names, lens, seqs, {"min_pct": 101}))
    assert e.value.code == api.E_ARG


# ---- the command line ----
def test_refusals_of_the_command_line(tmp_path):
    """before the index is read (the .ufi named here does not exist), each by the word that is wrong"""
    exe = os.path.join(ROOT, "urmap_amd", "urmap")
    fq, out, vcf = os.path.join(GOLD, "se150.fq"), str(tmp_path / "o.bam"), str(tmp_path / "o.vcf")
    fifo = str(tmp_path / "pipe")
    os.mkfifo(fifo)
    assert stat.S_ISFIFO(os.stat(fifo).st_mode)
    base = [exe, "-map", fq, "-ufi", str(tmp_path / "none.ufi"), "-bamout", out]
    for args, word in ((["-vcfout", vcf], "-vcfout needs -sort"), (["-sort", "-vcfout", ""], "-vcfout needs a file name"),
                       (["-sort", "-vcfout", out], "a file of their own"), (["-sort", "-vcfout", out + ".bai"], "a file of their own"),
                       (["-sort", "-depth", vcf, "-vcfout", vcf], "a file of their own"), (["-sort", "-stats", vcf, "-vcfout", vcf], "a file of their own"),
                       (["-sort", "-vcfout", fifo], "not a pipe"), (["-sort", "-vcfout", "/dev/stdout"], "not a pipe"),
                       (["-sort", "-vcf_mapq", "3"], "-vcf_mapq needs -vcfout"), (["-sort", "-vcf_baseq", "3"], "-vcf_baseq needs -vcfout"),
                       (["-sort", "-vcf_min_alt", "3"], "-vcf_min_alt needs -vcfout"), (["-sort", "-vcf_min_pct", "3"], "-vcf_min_pct needs -vcfout"),
                       (["-sort", "-vcfout", vcf, "-vcf_min_pct", "101"], "-vcf_min_pct 101"), (["-sort", "-vcfout", vcf, "-vcf_mapq", "256"], "-vcf_mapq 256"),
                       (["-sort", "-vcfout", vcf, "-vcf_baseq", "256"], "-vcf_baseq 256"), (["-sort", "-vcfout", vcf, "-vcf_min_alt", "0"], "-vcf_min_alt 0"),
                       (["-sort", "-vcfout", vcf, "-vcf_baseq", "-1"], "-vcf_baseq -1"), (["-sort", "-vcfout", vcf, "-vcf_min_alt", "x"], "-vcf_min_alt x")):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and word in r.stderr and "-vcf" in r.stderr and "none.ufi" not in r.stderr, (args, r.stderr)
        assert not os.path.exists(out) and not os.path.exists(vcf)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)  # (no command: the help text)
    assert "-vcfout FILE" in r.stdout + r.stderr and "-vcf_min_pct" in r.stdout + r.stderr
