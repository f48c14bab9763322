"""CPU: the oracle (oracle/liburmap_oracle.so) against the golden fixtures written by the reference binary
(tests/golden/make_golden.py), and against the reference binary itself when it is present."""
import filecmp
import gzip
import os

import numpy as np
import pytest

import oracle_lib as ol

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold_ufi(tmp_path_factory):
    d = tmp_path_factory.mktemp("gold")
    p = os.path.join(d, "g.ufi")
    with gzip.open(os.path.join(GOLD, "g.ufi.gz"), "rb") as z, open(p, "wb") as f:
        f.write(z.read())
    return p


def read_records(path):
    with open(path, "rb") as f:
        return [l for l in f.read().split(b"\n") if l and not l.startswith(b"@PG")]


@pytest.mark.parametrize("name", ["se150", "se250", "se_short"])
def test_oracle_sam_equals_reference_golden(gold_ufi, tmp_path, name):
    """urmap -map (map.cpp:27-67): every SAM record identical to what the reference wrote."""
    idx = ol.Index.load(gold_ufi)
    out = os.path.join(tmp_path, name + ".sam")
    idx.map_file_se(os.path.join(GOLD, name + ".fq"), out, threads=2)
    assert read_records(out) == read_records(os.path.join(GOLD, name + ".sam"))


@pytest.mark.parametrize("name", ["pe150", "pe100_noisy"])
def test_oracle_pe_sam_equals_reference_golden(gold_ufi, tmp_path, name):
    """urmap -map2 (map2.cpp:39-90; State2::Search4, FindPairs, ScanPair, AdjustTopHitsAndMapqs, SetSAM2): every
    record of both mates identical to what the reference wrote (flags, RNEXT/PNEXT, TLEN included)."""
    idx = ol.Index.load(gold_ufi)
    out = os.path.join(tmp_path, name + ".sam")
    idx.map_file_pe(os.path.join(GOLD, name + "_1.fq"), os.path.join(GOLD, name + "_2.fq"), out, threads=2)
    assert read_records(out) == read_records(os.path.join(GOLD, name + ".sam"))


def test_oracle_make_ufi_equals_reference_golden(gold_ufi, tmp_path):
    """urmap -make_ufi (ufindexio.cpp:117-179): byte-identical .ufi for the reference's slot count."""
    w, maxix, sds, slots = ol.ufi_header(gold_ufi)
    idx = ol.Index.build(os.path.join(GOLD, "g.fa"), slots, word_length=w, max_ix=maxix)
    out = os.path.join(tmp_path, "o.ufi")
    idx.save(out)
    assert filecmp.cmp(out, gold_ufi, shallow=False)


def test_viterbi_known_shapes():
    """The only worked cases in the reference tree are the three pairs in viterbi.cpp:286-302 (no expected
    values there); expected strings below were produced by the reference's State1::Viterbi semantics as pinned
    through the golden SAMs, and guard the Left/Right free-end-gap rules."""
    s, p = ol.viterbi(b"GGGGATTAC", b"GGGGATTACA", False, True)
    assert (s, p) == (9.0, "MMMMMMMMMI")
    s, p = ol.viterbi(b"GGATTACA", b"GGGGATTACA", True, False)
    assert (s, p) == (8.0, "IIMMMMMMMM")
    s, p = ol.viterbi(b"ACGT", b"", False, True)
    assert (s, p) == (-8.0, "DDDD")


def _sorted_records(path):
    return b"\n".join(sorted(read_records(path)))


def _sorted_pairs(path):
    body = [x for x in read_records(path) if not x.startswith(b"@")]
    return b"\n".join(sorted(body[i] + b"|" + body[i + 1] for i in range(0, len(body), 2)))


def _file_bytes(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("seed,glen,n,rl,sub,indel", [(21, 400000, 3000, 150, 0.01, 0.001),
                                                      (22, 300000, 1500, 250, 0.04, 0.01),
                                                      (23, 200000, 2000, 75, 0.02, 0.004)])
def test_oracle_equals_reference_binary(tmp_path, seed, glen, n, rl, sub, indel):
    """Fresh seeded genome + reads: reference -make_ufi / -map vs the oracle; .ufi bytes and SAM records (the reference's
    outputs as recorded in tests/golden/ref_runs.json when its binary is not built)."""
    from urmap_amd import synth
    d = str(tmp_path)
    g = synth.make_genome(seed, [glen * 6 // 10, glen * 3 // 10, glen // 10], repeat_frac=0.4, n_families=10)
    synth.write_fasta(os.path.join(d, "g.fa"), g, lowercase_frac=0.05)
    reads = synth.make_reads(seed + 1, g, n, read_len=rl, sub=sub, ins=indel / 2, dele=indel / 2, random_frac=0.02)
    rng = np.random.default_rng(seed)
    for k in range(0, len(reads), 29):
        lab, s, q = reads[k]
        s = s.copy(); s[int(rng.integers(0, len(s)))] = ord("N"); reads[k] = (lab, s, q)
    synth.write_fastq(os.path.join(d, "r.fq"), reads)
    # paired-end on the same genome
    r1, r2 = synth.make_pairs(seed + 2, g, n // 2, read_len=min(rl, 150), sub1=sub, sub2=2 * sub, ins=indel / 2, dele=indel / 2)
    synth.write_fastq(os.path.join(d, "p1.fq"), r1)
    synth.write_fastq(os.path.join(d, "p2.fq"), r2)

    def reference():
        ol.run_ref(["-make_ufi", "g.fa", "-output", "g.ufi"], cwd=d)
        ol.run_ref(["-map", "r.fq", "-ufi", "g.ufi", "-samout", "ref.sam", "-threads", "4"], cwd=d)
        ol.run_ref(["-map2", "p1.fq", "-reverse", "p2.fq", "-ufi", "g.ufi", "-samout", "refpe.sam", "-threads", "4"], cwd=d)
        return {"ufi_header": ol.ufi_header(os.path.join(d, "g.ufi")), "ufi": _file_bytes(os.path.join(d, "g.ufi")),
                "sam": _sorted_records(os.path.join(d, "ref.sam")), "pe_sam": _sorted_pairs(os.path.join(d, "refpe.sam"))}
    want = ol.reference_outputs(f"oracle_equals_reference_binary[{seed}]", reference)
    w, maxix, sds, slots = want["ufi_header"]
    idx = ol.Index.build(os.path.join(d, "g.fa"), slots)
    idx.save(os.path.join(d, "o.ufi"))
    assert ol.ufi_header(os.path.join(d, "o.ufi")) == tuple(want["ufi_header"])
    assert ol.digest(_file_bytes(os.path.join(d, "o.ufi"))) == want["ufi"]
    idx.map_file_se(os.path.join(d, "r.fq"), os.path.join(d, "o.sam"), threads=4)
    assert ol.digest(_sorted_records(os.path.join(d, "o.sam"))) == want["sam"]
    idx.map_file_pe(os.path.join(d, "p1.fq"), os.path.join(d, "p2.fq"), os.path.join(d, "ope.sam"), threads=4)
    assert ol.digest(_sorted_pairs(os.path.join(d, "ope.sam"))) == want["pe_sam"]


@pytest.mark.parametrize("name,ufi_gz,with_sam", [("pe150", "g.ufi.gz", True), ("pe100_noisy", "g.ufi.gz", True),
                                                  ("pe120_rep", "r.ufi.gz", True), ("pe120_rep", "r.ufi.gz", False)])
def test_oracle_tabbedout_equals_reference_golden(tmp_path, name, ufi_gz, with_sam):
    """State2::OutputTab2 (outputtab2.cpp:85-120) restated: every line of the reference's -tabbedout file, incl. the
    second pair and the TL/Score info string (pe120_rep), with and without SAM output switched on."""
    ufi = os.path.join(tmp_path, "x.ufi")
    with gzip.open(os.path.join(GOLD, ufi_gz), "rb") as z, open(ufi, "wb") as f:
        f.write(z.read())
    idx = ol.Index.load(ufi)
    tab = os.path.join(tmp_path, "o.tab")
    idx.map_file_pe_tab(os.path.join(GOLD, name + "_1.fq"), os.path.join(GOLD, name + "_2.fq"),
                        os.path.join(tmp_path, "o.sam") if with_sam else None, tab, threads=2)
    want = open(os.path.join(GOLD, name + (".tab" if with_sam else "_nosam.tab")), "rb").read()
    assert open(tab, "rb").read() == want
    if with_sam:
        assert ol.sam_records(os.path.join(tmp_path, "o.sam")) == \
            [l for l in open(os.path.join(GOLD, name + ".sam"), "rb").read().split(b"\n") if l]


@pytest.mark.parametrize("key,mode,name,minq", [("se150", "map", "se150", 10), ("se250", "map", "se250", 10),
                                                ("se_short", "map", "se_short", 10), ("pe150", "map2", "pe150", 10),
                                                ("pe100_noisy", "map2", "pe100_noisy", 10),
                                                ("pe100_noisy_minq3", "map2", "pe100_noisy", 3)])
def test_oracle_hitstats_equal_reference_report(gold_ufi, key, mode, name, minq):
    """UpdateHitStats (output1.cpp:20-30): no top hit -> unmapped, else MAPQ >= minq -> accepted, else rejected.  The
    oracle's per-read results give the counts the reference binary printed (tests/golden/hitstats.json)."""
    import json
    import re
    from urmap_amd import api
    want = json.load(open(os.path.join(GOLD, "hitstats.json")))[key]
    idx = ol.Index.load(gold_ufi)
    if mode == "map":
        _, bases, offs, _ = api.read_fastq_arrays(os.path.join(GOLD, name + ".fq"))
        res, _, _ = idx.map_se(bases, offs)
    else:
        _, bases, offs, _ = api.interleave_pairs(api.read_fastq_arrays(os.path.join(GOLD, name + "_1.fq")),
                                                 api.read_fastq_arrays(os.path.join(GOLD, name + "_2.fq")))
        res, _, _ = idx.map_pe(bases, offs)
    mapped = res["dbpos"] != 0xFFFFFFFF
    counts = [len(res), int((mapped & (res["mapq"] >= minq)).sum()), int((mapped & (res["mapq"] < minq)).sum()),
              int((~mapped).sum())]
    assert [int(re.match(r"\s*([\d,]+)", ln).group(1).replace(",", "")) for ln in want[:4]] == counts


@pytest.mark.parametrize("seed,maxix_opt", [(31, []), (32, ["-veryfast"])])
def test_oracle_veryfast_equals_reference_binary(tmp_path, seed, maxix_opt):
    """`-veryfast`: SE method 7 (state1.cpp:166-179) and PE Search5 (search2m5.cpp:9-156, band radius 4, map2.cpp:17-21),
    on a default index and on a `-make_ufi -veryfast` index (MaxIx 3, ufindexio.cpp:133-136): oracle vs reference SAM
    (the reference's outputs as recorded in tests/golden/ref_runs.json when its binary is not built)."""
    from urmap_amd import synth
    d = str(tmp_path)
    g = synth.make_genome(seed, [200000, 90000, 30000], repeat_frac=0.45, n_families=8, max_div=0.06)
    synth.write_fasta(os.path.join(d, "g.fa"), g, lowercase_frac=0.03)
    reads = synth.make_reads(seed + 1, g, 2500, read_len=150, sub=0.03, ins=0.003, dele=0.003, random_frac=0.02)
    synth.write_fastq(os.path.join(d, "r.fq"), reads)
    r1, r2 = synth.make_pairs(seed + 2, g, 1500, read_len=125, sub1=0.02, sub2=0.05, ins=0.002, dele=0.002)
    synth.write_fastq(os.path.join(d, "p1.fq"), r1)
    synth.write_fastq(os.path.join(d, "p2.fq"), r2)

    def reference():
        ol.run_ref(["-make_ufi", "g.fa", "-output", "g.ufi"] + maxix_opt, cwd=d)
        ol.run_ref(["-map", "r.fq", "-ufi", "g.ufi", "-samout", "ref.sam", "-threads", "4", "-veryfast"], cwd=d)
        ol.run_ref(["-map2", "p1.fq", "-reverse", "p2.fq", "-ufi", "g.ufi", "-samout", "refpe.sam", "-threads", "4", "-veryfast"], cwd=d)
        return {"ufi_header": ol.ufi_header(os.path.join(d, "g.ufi")), "ufi": _file_bytes(os.path.join(d, "g.ufi")),
                "sam": _sorted_records(os.path.join(d, "ref.sam")), "pe_sam": _sorted_pairs(os.path.join(d, "refpe.sam"))}
    want = ol.reference_outputs(f"oracle_veryfast_equals_reference_binary[{seed}]", reference)
    w, maxix, sds, slots = want["ufi_header"]
    assert maxix == (3 if maxix_opt else 32)
    idx = ol.Index.build(os.path.join(d, "g.fa"), slots, max_ix=maxix)
    idx.save(os.path.join(d, "o.ufi"))
    assert ol.ufi_header(os.path.join(d, "o.ufi")) == tuple(want["ufi_header"])
    assert ol.digest(_file_bytes(os.path.join(d, "o.ufi"))) == want["ufi"]
    idx.map_file_se(os.path.join(d, "r.fq"), os.path.join(d, "o.sam"), method=7, threads=4)
    assert ol.digest(_sorted_records(os.path.join(d, "o.sam"))) == want["sam"]
    idx.map_file_pe(os.path.join(d, "p1.fq"), os.path.join(d, "p2.fq"), os.path.join(d, "ope.sam"), threads=4, veryfast=True)
    assert ol.digest(_sorted_pairs(os.path.join(d, "ope.sam"))) == want["pe_sam"]


@pytest.mark.parametrize("seed,rl,sub", [(41, 279, 0.02), (42, 250, 0.05)])
def test_oracle_long_pairs_equal_reference_binary(tmp_path, seed, rl, sub):
    """Paired-end at the top of the reference's working range (pending seed positions are bytes, state1.h:86-87: the
    reference binary crashes from 2x280 on): oracle vs reference SAM on 250 and 279 bp pairs (the reference's outputs as
    recorded in tests/golden/ref_runs.json when its binary is not built)."""
    from urmap_amd import synth
    d = str(tmp_path)
    g = synth.make_genome(seed, [240000, 120000, 40000], repeat_frac=0.5, n_families=10, max_div=0.05)
    synth.write_fasta(os.path.join(d, "g.fa"), g)
    r1, r2 = synth.make_pairs(seed + 2, g, 1500, read_len=rl, sub1=sub, sub2=2 * sub, ins=0.002, dele=0.002)
    synth.write_fastq(os.path.join(d, "p1.fq"), r1)
    synth.write_fastq(os.path.join(d, "p2.fq"), r2)

    def reference():
        ol.run_ref(["-make_ufi", "g.fa", "-output", "g.ufi"], cwd=d)
        ol.run_ref(["-map2", "p1.fq", "-reverse", "p2.fq", "-ufi", "g.ufi", "-samout", "ref.sam", "-threads", "1"], cwd=d)
        return {"ufi_header": ol.ufi_header(os.path.join(d, "g.ufi")), "ufi": _file_bytes(os.path.join(d, "g.ufi")),
                "sam": b"\n".join(read_records(os.path.join(d, "ref.sam")))}
    want = ol.reference_outputs(f"oracle_long_pairs_equal_reference_binary[{seed}]", reference)
    # the index the reference wrote, rebuilt by the oracle byte for byte (test_oracle_equals_reference_binary)
    idx = ol.Index.build(os.path.join(d, "g.fa"), want["ufi_header"][3])
    idx.save(os.path.join(d, "o.ufi"))
    assert ol.digest(_file_bytes(os.path.join(d, "o.ufi"))) == want["ufi"]
    idx = ol.Index.load(os.path.join(d, "o.ufi"))
    idx.map_file_pe(os.path.join(d, "p1.fq"), os.path.join(d, "p2.fq"), os.path.join(d, "o.sam"), threads=4)
    assert ol.digest(b"\n".join(read_records(os.path.join(d, "o.sam")))) == want["sam"]


# ---------------------------------------------------------------------------------------------------------------------------
# letter classes (tests/alphabet_lib.py): N at the ends and in runs, lower case, IUPAC, U / u, letters without a complement,
# reads that keep the store's N -- in single reads and, independently, in both mates of a pair
# ---------------------------------------------------------------------------------------------------------------------------
def _alpha_golden_sets(gold_ufi):
    """the generator's output for the golden sets again (it is a pure function of the seed), with the tags"""
    import alphabet_lib as al
    store = al.Store(ol.Index.load(gold_ufi), os.path.join(GOLD, "g.fa"))
    reads, tags = al.make_reads(31, store, 560, read_len=150)
    r1, r2, t1, t2 = al.make_pairs(32, store, 300, read_len=150)
    return reads, tags, r1, r2, t1, t2


def _alpha(name, tmp_path=None):
    """an alpha fixture (kept .gz): its bytes, or -- with tmp_path -- the path of an unpacked copy"""
    with gzip.open(os.path.join(GOLD, name + ".gz"), "rb") as z:
        data = z.read()
    if tmp_path is None:
        return data
    p = os.path.join(tmp_path, name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def _fastq_bytes(reads):
    return b"".join(b"@" + lab.encode() + b"\n" + s.tobytes() + b"\n+\n" + q.tobytes() + b"\n" for lab, s, q in reads)


def test_oracle_alpha_sam_equals_reference_golden(gold_ufi, tmp_path):
    """se_alpha: 560 reads, 40 of each letter class.  The oracle's SAM is the reference's, byte for byte; every class that can map
    has at least 20 mapped reads in the oracle's results (the oracle reaches: see the assertion message of check_classes)."""
    import alphabet_lib as al
    from conftest import reads_to_arrays
    reads, tags = _alpha_golden_sets(gold_ufi)[:2]
    assert _fastq_bytes(reads) == _alpha("se_alpha.fq")  # the tags belong to the file's reads
    idx = ol.Index.load(gold_ufi)
    out = os.path.join(tmp_path, "o.sam")
    idx.map_file_se(_alpha("se_alpha.fq", tmp_path), out, threads=2)
    assert read_records(out) == [l for l in _alpha("se_alpha.sam").split(b"\n") if l]
    bases, offs = reads_to_arrays(reads)
    ores, _, _ = idx.map_se(bases, offs)
    cc = al.check_classes(tags, ores, np.diff(offs.astype(np.int64)), min_exact=1)  # 40 case_kept reads on a 40 kbp genome
    print("se_alpha (reads, mapped) per class:", cc)
    assert {t["kind"] for t in tags} == set(al.KINDS)


def test_oracle_alpha_pairs_equal_reference_golden(gold_ufi, tmp_path):
    """pe_alpha: 300 pairs, the class of each mate drawn on its own.  SAM and -tabbedout lines of the oracle are the reference's,
    byte for byte; all nine (plain, four-plane, other)^2 mate combinations occur at least 10 times and at least 30 proper pairs have
    a mate 2 that is not plain."""
    import alphabet_lib as al
    from conftest import reads_to_arrays
    _, _, r1, r2, t1, t2 = _alpha_golden_sets(gold_ufi)
    assert _fastq_bytes(r1) == _alpha("pe_alpha_1.fq")
    assert _fastq_bytes(r2) == _alpha("pe_alpha_2.fq")
    idx = ol.Index.load(gold_ufi)
    sam, tab = os.path.join(tmp_path, "o.sam"), os.path.join(tmp_path, "o.tab")
    idx.map_file_pe_tab(_alpha("pe_alpha_1.fq", tmp_path), _alpha("pe_alpha_2.fq", tmp_path), sam, tab, threads=2)
    assert _file_bytes(tab) == _alpha("pe_alpha.tab")
    assert ol.sam_records(sam) == [l for l in _alpha("pe_alpha.sam").split(b"\n") if l]
    combos, proper = al.check_pair_kinds(t1, t2, _alpha("pe_alpha.sam"))
    bases, offs = reads_to_arrays([x for ab in zip(r1, r2) for x in ab])
    ores, _, _ = idx.map_pe(bases, offs)
    cc = al.check_classes([x for ab in zip(t1, t2) for x in ab], ores, np.diff(offs.astype(np.int64)), min_exact=1)
    print("pe_alpha pairs per (kind of mate 1, kind of mate 2):", combos, "proper pairs with a non-plain mate 2:", proper)
    print("pe_alpha (mates, mapped) per class:", cc)


@pytest.mark.parametrize("veryfast", [False, True])
def test_oracle_alphabet_equals_reference_binary(tmp_path, veryfast):
    """A fresh genome with soft-masked stretches and N runs, 2 800 single reads and 1 500 pairs in the letter classes, default and
    -veryfast (on a MaxIx 3 index): oracle vs reference SAM (the reference's outputs as recorded in tests/golden/ref_runs.json
    when its binary is not built).  Then the same index with the FASTA's case put back into its sequence store
    (alphabet_lib.soft_masked_index), where reads that keep the store's case have to match lower case against lower case: the
    reference binary takes that .ufi as it is."""
    import alphabet_lib as al
    from urmap_amd import synth
    d = str(tmp_path)
    g = synth.make_genome(51, [200000, 90000, 30000], repeat_frac=0.4, n_families=10, n_run_frac=0.02)
    fa = os.path.join(d, "g.fa")
    synth.write_fasta(fa, g, lowercase_frac=0.06, seed=5)
    vf = ["-veryfast"] if veryfast else []
    slots = 524309
    idx = ol.Index.build(fa, slots, max_ix=3 if veryfast else 32)
    idx.save(os.path.join(d, "o.ufi"))
    soft = al.soft_masked_index(idx, fa)
    soft.save(os.path.join(d, "soft.ufi"))
    inputs = {}
    for name, oi in (("hard", idx), ("soft", soft)):
        store = al.Store(oi, fa)
        reads, tags = al.make_reads(52, store, 2800, read_len=150, sub=0.02, indel=0.002)
        r1, r2, t1, t2 = al.make_pairs(53, store, 1500, read_len=125, sub1=0.02, sub2=0.04, indel=0.002)
        synth.write_fastq(os.path.join(d, name + "_r.fq"), reads)
        synth.write_fastq(os.path.join(d, name + "_1.fq"), r1)
        synth.write_fastq(os.path.join(d, name + "_2.fq"), r2)
        inputs[name] = (reads, tags, r1, r2, t1, t2)

    def reference():
        ol.run_ref(["-make_ufi", "g.fa", "-output", "g.ufi", "-slots", str(slots)] + vf, cwd=d)
        out = {"ufi": _file_bytes(os.path.join(d, "g.ufi"))}
        for name, ufi in (("hard", "g.ufi"), ("soft", "soft.ufi")):
            ol.run_ref(["-map", name + "_r.fq", "-ufi", ufi, "-samout", name + ".sam", "-threads", "1"] + vf, cwd=d)
            ol.run_ref(["-map2", name + "_1.fq", "-reverse", name + "_2.fq", "-ufi", ufi, "-samout", name + "_pe.sam", "-tabbedout",
                        name + "_pe.tab", "-threads", "1"] + vf, cwd=d)
            out[name + "_sam"] = b"\n".join(read_records(os.path.join(d, name + ".sam")))
            out[name + "_pe_sam"] = b"\n".join(read_records(os.path.join(d, name + "_pe.sam")))
            out[name + "_pe_tab"] = _file_bytes(os.path.join(d, name + "_pe.tab"))
        return out
    want = ol.reference_outputs(f"oracle_alphabet_equals_reference_binary[{'veryfast' if veryfast else 'default'}]", reference)
    assert ol.digest(_file_bytes(os.path.join(d, "o.ufi"))) == want["ufi"]
    from conftest import reads_to_arrays
    for name, oi in (("hard", idx), ("soft", soft)):
        reads, tags, r1, r2, t1, t2 = inputs[name]
        osam, opsam, otab = (os.path.join(d, name + x) for x in ("_o.sam", "_ope.sam", "_ope.tab"))
        oi.map_file_se(os.path.join(d, name + "_r.fq"), osam, method=7 if veryfast else 6, threads=4)
        assert ol.digest(b"\n".join(read_records(osam))) == want[name + "_sam"], name
        oi.map_file_pe_tab(os.path.join(d, name + "_1.fq"), os.path.join(d, name + "_2.fq"), opsam, otab, threads=4, veryfast=veryfast)
        assert ol.digest(b"\n".join(read_records(opsam))) == want[name + "_pe_sam"], name
        assert ol.digest(_file_bytes(otab)) == want[name + "_pe_tab"], name
        bases, offs = reads_to_arrays(reads)
        ores, _, _ = oi.map_se(bases, offs, method=7 if veryfast else 6, threads=4)
        cc = al.check_classes(tags, ores, np.diff(offs.astype(np.int64)))
        combos, proper = al.check_pair_kinds(t1, t2, _file_bytes(opsam))
        print(name, "veryfast" if veryfast else "default", "(reads, mapped) per class:", cc, "pairs per kind combination:", combos,
              "proper pairs with a non-plain mate 2:", proper)
        if name == "soft":  # lower case has to match lower case here
            assert sum(1 for t in tags if t["cls"] == "case_kept" and t["lower"] and t["kind"] == "four") >= 20
