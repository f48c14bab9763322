"""Optional fields NM, MD, AS, RG on the host: the pure NM/MD function and the four tagged formatters against the spec-level
yardstick of tests/tags_lib.py -- on the reference-written goldens (results from the oracle) and on hand-made alignments over a
wrapped host index --, the -tags / -rg refusals of the command line, the @RG line's place in the headers, the span call over host
arrays, and the tagged host formatters inside the sanitizer program."""
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bam_lib as bl
import edges_lib as el
import oracle_lib as ol
import tags_lib as tl
from test_abi_cpu import oracle_results_as_product
from urmap_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SAN_DIR = os.path.join(ROOT, "urmap_amd", "csrc", "build_san")
URMAP = os.path.join(ROOT, "urmap_amd", "urmap")
RG_LINE, RG_ID = "@RG\tID:grp.1\tSM:s1\tPL:ILLUMINA", "grp.1"
ALL = {"NM", "MD", "AS"}

# name -> (paired, index, FASTA)
GOLDENS = {"se150": (False, "g", "g.fa"), "se250": (False, "g", "g.fa"), "se_short": (False, "g", "g.fa"), "se_alpha": (False, "g", "g.fa"),
           "pe150": (True, "g", "g.fa"), "pe100_noisy": (True, "g", "g.fa"), "pe_alpha": (True, "g", "g.fa"), "pe120_rep": (True, "r", "r.fa"),
           "edges_se": (False, "edges", "edges.fa"), "geometry": (True, "geometry", "geometry.fa")}


def gold(name):
    p = os.path.join(GOLD, name)
    if os.path.exists(p):
        return open(p, "rb").read()
    with gzip.open(p + ".gz", "rb") as z:
        return z.read()


@pytest.fixture(scope="module")
def ufis(tmp_path_factory):
    d = tmp_path_factory.mktemp("tags_ufi")
    out = {}
    for name in ("g", "r"):
        out[name] = os.path.join(d, name + ".ufi")
        with gzip.open(os.path.join(GOLD, name + ".ufi.gz"), "rb") as z, open(out[name], "wb") as f:
            f.write(z.read())
    for name in ("edges", "geometry"):
        out[name] = os.path.join(d, name + ".ufi")
        ol.Index.build(os.path.join(GOLD, name + ".fa"), el.SLOTS).save(out[name])
    return out


def fastq_arrays(name, d):
    p = os.path.join(GOLD, name)
    if not os.path.exists(p):
        p = os.path.join(d, name)
        open(p, "wb").write(gold(name))
    return api.read_fastq_arrays(p)


_mapped = {}


def golden_batch(name, ufis, d):
    """the golden's reads and the oracle's results in the product's layout, computed once per golden"""
    if name not in _mapped:
        paired, ufi, fa = GOLDENS[name]
        if paired:
            reads = api.interleave_pairs(fastq_arrays(name + "_1.fq", d), fastq_arrays(name + "_2.fq", d))
            ores, opaths, _ = ol.Index.load(ufis[ufi]).map_pe(reads[1], reads[2], threads=4)
        else:
            reads = fastq_arrays(name + ".fq", d)
            ores, opaths, _ = ol.Index.load(ufis[ufi]).map_se(reads[1], reads[2], threads=4)
        res, ops = oracle_results_as_product(ores, opaths)
        res.setflags(write=False)
        _mapped[name] = (reads, res, ops, tl.read_fasta(os.path.join(GOLD, fa)))
    return _mapped[name]


# ---- the yardstick checks itself on values worked out by hand from the SAMtags text ----
def test_tags_lib_by_hand():
    ref = "ACGTACGTAC"
    assert tl.calmd(ref, 1, "10M", "ACGTACGTAC") == (0, "10")
    assert tl.calmd(ref, 1, "10M", "TCGTACGTAG") == (2, "0A8C0")
    assert tl.calmd(ref, 1, "3M2D5M", "ACGCGTAC") == (2, "3^TA5")
    assert tl.calmd(ref, 1, "3M2D5M", "ACGAGTAC") == (3, "3^TA0C4")      # a deletion, then a mismatch: the 0 stays
    assert tl.calmd(ref, 1, "2D8M", "GTACGTAC") == (2, "0^AC8")           # a CIGAR that begins with D
    assert tl.calmd(ref, 1, "3M2I7M", "ACGGGTACGTAC") == (2, "10")        # an insertion neither prints nor resets
    assert tl.calmd("ANNRA", 1, "5M", "ANnRa") == (2, "1N0N2")            # N never matches, R matches R, case never matters
    assert tl.calmd("acgt", 2, "2M", "CA") == (1, "1G0")
    tl.check_against_fasta(ref, 1, "ACGAGTAC", "3M2D5M", "3^TA0C4")
    with pytest.raises(AssertionError):
        tl.check_against_fasta(ref, 1, "ACGAGTAC", "3M2D5M", "3^TT0C4")
    with pytest.raises(AssertionError):
        tl.rebuild_reference("ACGT", "4M", "5")
    assert [tl.smallest_int_type(v) for v in (0, 255, 256, 65535, 65536, -1, -128, -129, -32768, -32769)] == list("CCSSIccssi")
    assert tl.parse_aux(b"NMC\x05MDZ3^TA0C4\0ASs\xfe\xffRGZx\0") == [("NM", "C", 5), ("MD", "Z", "3^TA0C4"), ("AS", "s", -2), ("RG", "Z", "x")]


def test_calmd_entry_point():
    assert api.calmd(b"ACGTACGTAC", [(3, "M"), (2, "D"), (5, "M")], b"ACGAGTAC") == (3, "3^TA0C4")
    assert api.calmd(b"ANNRA", [(5, "M")], b"ANnRa") == (2, "1N0N2")
    assert api.calmd(b"", [(3, "I")], b"ACG") == (3, "0")
    for ref, cigar, seq in ((b"ACG", [(4, "M")], b"ACGT"), (b"ACGT", [(4, "M")], b"ACG"), (b"ACG", [(2, "M"), (2, "D")], b"AC")):
        with pytest.raises(ValueError):
            api.calmd(ref, cigar, seq)


# ---- the goldens ----
@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_tagged_formatters_on_the_goldens(ufis, tmp_path_factory, name):
    d = tmp_path_factory.mktemp("fq")
    (labels, bases, offs, quals), res, ops, fasta = golden_batch(name, ufis, d)
    paired = GOLDENS[name][0]
    idx = api.Index.open(ufis[GOLDENS[name][1]])
    want = [l for l in gold(name + ".sam").decode("latin-1").split("\n") if l and not l.startswith("@")]
    sam = idx.records_tags(res, ops, labels, bases, offs, quals, tags=api.TAG_ALL, rg_id=RG_ID, paired=paired).decode("latin-1")
    lines = [l for l in sam.split("\n") if l]
    assert len(lines) == len(want) == len(res)
    n_mapped = n_gapped = 0
    for i, line in enumerate(lines):
        assert tl.check_sam_record(line, fasta, ALL, RG_ID, score=res["score"][i]) == want[i]  # cut off, it is the golden line
        f = line.split("\t")
        if f[2] == "*":
            assert f[11:] == ["RG:Z:" + RG_ID]
        else:
            n_mapped += 1
            n_gapped += "I" in f[5] or "D" in f[5]
    assert n_mapped > 0
    # without options: the bytes of the functions that take none
    plain = idx.sam_pe(res, ops, labels, bases, offs, quals) if paired else idx.sam_se(res, ops, labels, bases, offs, quals)
    assert idx.records_tags(res, ops, labels, bases, offs, quals, paired=paired) == plain
    # BAM: the same values as aux fields in the same order, the smallest integer types, block_size over all of it
    refs = [(n, ln) for n, ln, _ in idx.directory()]
    bam = idx.records_tags(res, ops, labels, bases, offs, quals, tags=api.TAG_ALL, rg_id=RG_ID, bam=True, paired=paired)
    recs = tl.read_bam_records_aux(bam, refs)
    assert len(recs) == len(lines)
    for (bline, aux), line in zip(recs, lines):
        base, tags, order = tl.split_fields(line)
        assert bline == bl.normalise_sam_line(base)
        assert aux == tl.aux_of_sam_fields(tags, order)
    plain_bam = idx.bam_pe(res, ops, labels, bases, offs, quals) if paired else idx.bam_se(res, ops, labels, bases, offs, quals)
    assert idx.records_tags(res, ops, labels, bases, offs, quals, bam=True, paired=paired) == plain_bam
    assert [b for b, _ in recs] == bl.read_bam_records(plain_bam, refs)


def test_goldens_hold_the_hard_cases(ufis, tmp_path_factory):
    """what the issue counts on being there: gap runs at a CIGAR's ends, ^..0X, records wholly inside an N run, lower-case reference"""
    d = tmp_path_factory.mktemp("fq2")
    seen = {"edge_gap": 0, "del_then_mm": 0, "all_n": 0, "minus_gapped": 0}
    for name in ("pe100_noisy", "pe120_rep", "se_alpha"):
        (labels, bases, offs, quals), res, ops, fasta = golden_batch(name, ufis, d)
        idx = api.Index.open(ufis[GOLDENS[name][1]])
        sam = idx.records_tags(res, ops, labels, bases, offs, quals, tags=api.TAG_ALL, paired=GOLDENS[name][0]).decode("latin-1")
        for i, line in enumerate(l for l in sam.split("\n") if l):
            f = line.split("\t")
            if f[2] == "*":
                continue
            _, tags, _ = tl.split_fields(line)
            cig = bl.parse_cigar(f[5])
            seen["edge_gap"] += cig[0][1] != "M" or cig[-1][1] != "M"
            seen["del_then_mm"] += bool(re.search(r"\^[A-Z]+0[A-Z]", tags["MD"][1]))
            seen["all_n"] += len(cig) == 1 and int(tags["NM"][1]) == len(f[9])
            seen["minus_gapped"] += len(cig) > 1 and not res["plus"][i]
    assert all(seen.values()), seen
    g = tl.read_fasta(os.path.join(GOLD, "g.fa"))
    assert any(c.islower() for seq in g.values() for c in seq)


# ---- hand-made alignments on a wrapped host index ----
@pytest.fixture(scope="module")
def hand():
    store = tl.hand_store()
    cases = tl.hand_cases(store)
    seq = np.frombuffer(store.encode(), dtype=np.uint8)
    blob = np.zeros(5 * 101 + 8, dtype=np.uint8)
    idx = api.Index.wrap_host(24, 32, 101, blob, seq, [len(store)], [0], ["c"])
    return {"store": store, "cases": cases, "idx": idx, "batch": tl.hand_batch(cases)}


def test_hand_made_alignments(hand):
    idx, cases, store = hand["idx"], hand["cases"], hand["store"]
    bases, offs, res, ops = hand["batch"]
    labels = [c["name"] for c in cases]
    quals = np.full(len(bases), 73, np.uint8)
    sam = idx.records_tags(res, ops, labels, bases, offs, quals, tags=api.TAG_ALL, rg_id=RG_ID).decode("latin-1")
    plain = idx.records_tags(res, ops, labels, bases, offs, quals).decode("latin-1")
    lines, plain_lines = [l for l in sam.split("\n") if l], [l for l in plain.split("\n") if l]
    fasta = {"c": store}
    by_name = {}
    for c, line, pl, r in zip(cases, lines, plain_lines, res):
        assert tl.check_sam_record(line, fasta, ALL, RG_ID, score=r["score"]) == pl, c["name"]
        f = line.split("\t")
        assert f[9] == c["printed"], c["name"]
        by_name[c["name"]] = (f[5], tl.split_fields(line)[1])
    md = lambda n: by_name[n][1]["MD"][1]
    nm = lambda n: int(by_name[n][1]["NM"][1])
    # what these shapes are there for, said once in plain values
    assert md("cols64") == "64" and md("cols65") == "65" and md("cols1") == "1"
    assert md("cols1_mm_ends") == "0" + store[5000] + "0"
    assert md("cols65_mm_ends") == "0" + store[5000] + "63" + store[5064] + "0"
    assert md("mm_0_63_64_last") == f"0{store[6000]}62{store[6063]}0{store[6064]}134{store[6199]}0"
    assert by_name["run_across_step_and_I"][0] == "10M7I150M" and md("run_across_step_and_I") == f"3{store[6003]}156"
    assert md("D_then_mismatch") == f"40^{store[6040:6042]}0{store[6042]}59"
    assert by_name["starts_with_D"][0] == "6D101M" and md("starts_with_D").startswith("0^") and nm("starts_with_D") >= 6
    assert by_name["starts_with_I"][0] == "6I102M" and nm("starts_with_I") >= 6
    assert by_name["ends_with_D"][0].endswith("D")
    assert nm("N_against_N") == 70 and md("N_against_N") == "0N" * 70 + "0"
    assert nm("R_against_R") == 0 and md("R_against_R") == "40"
    assert nm("A_against_R") == 1 and md("A_against_R") == "12R27"
    assert nm("lower_case_read") == 0 and nm("lower_case_store") == 2 and md("lower_case_store").isupper()
    assert len(bl.parse_cigar(by_name["many_runs"][0])) > 96
    # BAM: the integer widths
    bam = idx.records_tags(res, ops, labels, bases, offs, quals, tags=api.TAG_ALL, rg_id=RG_ID, bam=True)
    recs = tl.read_bam_records_aux(bam, [("c", len(store))])
    types = {}
    for c, (bline, aux), line in zip(cases, recs, lines):
        base, tags, order = tl.split_fields(line)
        assert bline == bl.normalise_sam_line(base) and aux == tl.aux_of_sam_fields(tags, order), c["name"]
        types[c["name"]] = {t: ty for t, ty, _ in aux}
    assert [types[f"nm{n}"]["NM"] for n in (255, 256, 65535, 65536, 70000)] == ["C", "S", "S", "I", "I"]
    assert nm("nm70000") == 70000 and nm("nm65536") == 65536
    assert {ty["AS"] for ty in types.values()} >= {"C", "S", "c"}


@pytest.mark.parametrize("tags,rg", [(api.TAG_NM, None), (api.TAG_MD, None), (api.TAG_AS, None), (0, RG_ID), (api.TAG_NM | api.TAG_AS, RG_ID)])
def test_each_field_alone(hand, tags, rg):
    idx, cases = hand["idx"], hand["cases"][:20]
    bases, offs, res, ops = tl.hand_batch(cases)
    labels = [c["name"] for c in cases]
    quals = np.full(len(bases), 73, np.uint8)
    want = {n for n, b in (("NM", api.TAG_NM), ("MD", api.TAG_MD), ("AS", api.TAG_AS)) if tags & b}
    sam = idx.records_tags(res, ops, labels, bases, offs, quals, tags=tags, rg_id=rg).decode("latin-1")
    for line, r in zip([l for l in sam.split("\n") if l], res):
        tl.check_sam_record(line, {"c": hand["store"]}, want, rg, score=r["score"])
    bam = idx.records_tags(res, ops, labels, bases, offs, quals, tags=tags, rg_id=rg, bam=True)
    for (bline, aux), line in zip(tl.read_bam_records_aux(bam, [("c", len(hand["store"]))]), [l for l in sam.split("\n") if l]):
        base, t, order = tl.split_fields(line)
        assert aux == tl.aux_of_sam_fields(t, order)


def test_windows_in_place_of_the_host_store(hand):
    """the formatters given each record's reference window (what the span call returns) write the bytes they write from the store"""
    idx, cases = hand["idx"], hand["cases"]
    bases, offs, res, ops = hand["batch"]
    labels = [c["name"] for c in cases]
    quals = np.full(len(bases), 73, np.uint8)
    spans = [api.ref_span(res[i:i + 1], ops, int(offs[i + 1] - offs[i])) for i in range(len(res))]
    wins = idx.fetch_spans([int(r["coord"]) for r in res], spans)
    for bam in (False, True):
        assert idx.records_tags(res, ops, labels, bases, offs, quals, tags=api.TAG_ALL, rg_id=RG_ID, bam=bam, windows=wins) == \
               idx.records_tags(res, ops, labels, bases, offs, quals, tags=api.TAG_ALL, rg_id=RG_ID, bam=bam)


def test_span_call_over_host_arrays(hand):
    idx, store = hand["idx"], hand["store"].encode()
    n = len(store)
    starts, lens = [0, 0, 5, n - 1, n - 1, n, 1234, 0], [0, 1, 64, 1, 0, 0, 4321, n]
    got = idx.fetch_spans(starts, lens)
    assert got == [store[s:s + l] for s, l in zip(starts, lens)]
    assert idx.fetch_spans([], []) == []
    for s, l in ((n, 1), (n - 1, 2), (n + 1, 0), (0, n + 1)):
        with pytest.raises(api.UrmapxError):
            idx.fetch_spans([s], [l])


# ---- headers ----
def test_read_group_line_in_the_headers(hand):
    idx = hand["idx"]
    cl = "urmap -map x.fq -rg '@RG\\tID:grp.1' "
    pg = b"@PG\tID:urmap\tPN:urmap\tVN:1.0.mi355x\tCL:" + cl.encode() + b"\n"
    sq = idx.sam_header_sq()
    assert idx.header_rg(cl, RG_LINE) == sq + RG_LINE.encode() + b"\n" + pg
    assert idx.header_rg(cl, None) == sq + pg
    assert idx.header_rg(cl, RG_LINE, sorted=True) == b"@HD\tVN:1.6\tSO:coordinate\n" + sq + RG_LINE.encode() + b"\n" + pg
    text, refs, recs = bl.read_bam(idx.header_rg(cl, RG_LINE, bam=True))
    assert text == sq + RG_LINE.encode() + b"\n" + pg and refs == [("c", len(hand["store"]))] and recs == []
    text, _, _ = bl.read_bam(idx.header_rg(cl, RG_LINE, sorted=True, bam=True))
    assert [l.split("\t")[0] for l in text.decode().split("\n") if l] == ["@HD", "@SQ", "@RG", "@PG"]
    assert idx.header_rg(cl, None, bam=True) == idx.bam_header(cl)


# ---- -rg / -tags parsing ----
def test_read_group_parsing():
    assert api.read_group_id("@RG\\tID:a\\tSM:b") == ("@RG\tID:a\tSM:b", "a")
    assert api.read_group_id("@RG\tSM:b\tID:x y") == ("@RG\tSM:b\tID:x y", "x y")
    assert api.read_group_id("@RG\\tSM:b\tID:q\\tPL:z") == ("@RG\tSM:b\tID:q\tPL:z", "q")
    for line, word in (("RG\\tID:a", "must start with @RG"), ("@RGX\\tID:a", "must start with @RG"), ("@RG ID:a", "must start with @RG"),
                       ("@RG\\tSM:b", "no ID: field"), ("@RG\\tXID:b", "no ID: field"), ("@RG\\tID:\\tSM:b", "ID is empty"), ("@RG\\tID:", "ID is empty"),
                       ("@RG\\tID:a\nb", "newline"), ("@RG\\tID:a\\tSM:b\n", "newline")):
        with pytest.raises(ValueError) as e:
            api.read_group_id(line)
        assert word in str(e.value), (line, str(e.value))


def cli(*args):
    return subprocess.run([URMAP, "-map", os.path.join(GOLD, "se150.fq"), "-ufi", "/nonexistent/index.ufi"] + list(args), capture_output=True, text=True)


@pytest.mark.parametrize("args,word", [
    (["-samout", "o.sam", "-tags", "NM,XS"], "'XS'"), (["-samout", "o.sam", "-tags", "NM,MD,NM"], "'NM' is named twice"),
    (["-samout", "o.sam", "-tags", "NM,,MD"], "empty element"), (["-samout", "o.sam", "-tags", ""], "empty element"),
    (["-samout", "o.sam", "-tags", "NM,"], "empty element"), (["-samout", "o.sam", "-tags", "nm"], "'nm'"),
    (["-samout", "o.sam", "-rg", "RG\\tID:a"], "must start with @RG"), (["-samout", "o.sam", "-rg", "@RG\\tSM:a"], "no ID: field"),
    (["-samout", "o.sam", "-rg", "@RG\\tID:"], "ID is empty"), (["-samout", "o.sam", "-rg", "@RG\\tID:a\nb"], "newline"),
    (["-tags", "NM"], "-samout or -bamout")])
def test_cli_refuses_before_the_index_is_loaded(args, word):
    r = cli(*args)
    assert r.returncode != 0 and word in r.stderr and "index.ufi" not in r.stderr, r.stderr


def test_cli_takes_well_formed_options_as_far_as_the_index():
    r = cli("-samout", "o.sam", "-tags", "AS,NM,MD", "-rg", "@RG\\tID:a\\tSM:b")
    assert r.returncode != 0 and "index.ufi" in r.stderr, r.stderr


def test_options_struct_in_step():
    import ctypes as C
    assert [n for n, _ in api.MapOptions._fields_][-2:] == ["tags", "read_group"]
    assert C.sizeof(api.MapOptions) == 72 and api.MapOptions.tags.offset == 60 and api.MapOptions.read_group.offset == 64
    assert C.sizeof(api.TagOptions) == 32


# ---- the tagged host formatters and the span call inside the sanitizer program ----
@pytest.fixture(scope="module")
def san():
    if not shutil.which("g++"):
        pytest.skip("no g++ for the sanitizer builds")
    r = subprocess.run(["make", "-s", "-j3", "-C", os.path.join(ROOT, "urmap_amd", "csrc"), "san"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    return {k: os.path.join(SAN_DIR, "urmap_san_" + k) for k in ("asan", "tsan")}


@pytest.mark.parametrize("build,extra", [("asan", []), ("asan", ["-bam"]), ("asan", ["-2"]), ("asan", ["-bam", "-sort"]), ("tsan", ["-batch", "64", "-streams", "3"])])
def test_pipeline_tags_under_sanitizers(tmp_path, san, build, extra):
    """urmapx_map_files with tags and a read group, device side replaced by the stand-in: the lanes' chunks (the stand-in runs the host
    formatters), the host road reading the store, and the host road fed by the span call give the same tagged records"""
    paired = "-2" in extra
    fq = os.path.join(GOLD, "pe150_1.fq" if paired else "se150.fq")
    extra = [os.path.join(GOLD, "pe150_2.fq") if x == "__" else x for x in (["-2", "__"] if paired else extra)]
    bam = "-bam" in extra
    env = dict(os.environ, URX_STUB_MAP="1", ASAN_OPTIONS="exitcode=99:detect_leaks=0", UBSAN_OPTIONS="exitcode=99:halt_on_error=1",
               TSAN_OPTIONS="exitcode=99")
    common = extra + ["-biglen", "3000000", "-tags", "7", "-rg", RG_LINE]
    outs = {}
    for key, more_env in (("lanes", {}), ("host_store", {"URMAPX_HOST_TEXT": "1"}), ("host_spans", {"URMAPX_HOST_TEXT": "1", "URX_STUB_NO_HOST_SEQ": "1"})):
        out = str(tmp_path / (key + ".out"))
        r = subprocess.run([san[build], "map", fq, "-o", out] + common, env=dict(env, **more_env), capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        blob = open(out, "rb").read()
        outs[key] = bl.inflate(blob) if bam else blob
    if bam:
        text, refs, recs, _ = tl.read_bam_aux(outs["lanes"])
        assert ("@HD" in text.decode()) == ("-sort" in extra) and "\n" + RG_LINE + "\n@PG" in text.decode()
        body = {k: tl.read_bam_aux(v)[3] for k, v in outs.items()}
        assert len(recs) >= 400 and all(aux[-1] == ("RG", "Z", RG_ID) for _, aux in recs)
        assert any(len(aux) == 4 for _, aux in recs) and any(len(aux) == 1 for _, aux in recs)
        assert body["lanes"] == body["host_store"] == body["host_spans"]
    else:
        strip_pg = lambda b: b"\n".join(l for l in b.split(b"\n") if not l.startswith(b"@PG"))
        assert strip_pg(outs["lanes"]) == strip_pg(outs["host_store"]) == strip_pg(outs["host_spans"])
        lines = [l for l in outs["lanes"].decode("latin-1").split("\n") if l]
        hdr = [l for l in lines if l.startswith("@")]
        assert [h[:3] for h in hdr] == ["@SQ"] * 3 + ["@RG", "@PG"] and hdr[3] == RG_LINE
        recs = [l for l in lines if not l.startswith("@")]
        assert len(recs) >= 400
        n_tagged = 0
        for l in recs:
            _, tags, order = tl.split_fields(l)
            assert order in (["NM", "MD", "AS", "RG"], ["RG"]) and tags["RG"] == ("Z", RG_ID)
            n_tagged += len(order) == 4
        assert 0 < n_tagged < len(recs)
