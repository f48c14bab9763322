"""GPU: reads and pairs at the first and last bases of sequences and of the sequence store (tests/edges_lib.py), on every road
through the kernels.

AlignHSP's window arithmetic at the edges (alignhsp.cpp:98-150) is written out five times on the device -- kernels.hip:
SearchWave::align_hsp and dp_kernel, slow_dev.h: align_hsp, kernels_pe.hip: align_hsp, kernels_pe_slow.hip through slow_dev.h --,
ExtendPen's SeedPosDB < SeedPosQ and the walk into the zero bytes behind the store in the fast and the general form, ScanPair's
DBPos >= 1024 guard and its unclipped windows in both pair kernels.  Every result field and the full path are compared with the
oracle, which tests/test_edges_cpu.py pins to the reference binary on the reference-defined subset of the same lists; outside that
subset (cases whose walks or windows reach bytes behind the store) the oracle's 4 096 zero bytes are the definition being pinned.
That module also asserts, on the oracle alone, that the lists reach every edge branch and produce both outcomes at every edge.
"""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bam_lib as bl
import edges_lib as el
import oracle_lib as ol
from conftest import reads_to_arrays
from test_gpu_parity import compare_results
from urmap_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "urmap_amd", "urmap")


def _by_length(reads, pairs=False):
    """{length class: indices of the reads (pairs: by the longer mate)}: the kernels pick their instance by a batch's longest read"""
    out = {}
    step = 2 if pairs else 1
    for i in range(0, len(reads), step):
        out.setdefault(max(len(r[1]) for r in reads[i:i + step]), []).append(i // step)
    return out


@pytest.fixture(scope="module")
def edges(tmp_path_factory):
    """both stores as .ufi (the oracle's -make_ufi), every list with the oracle's results, computed once"""
    d = str(tmp_path_factory.mktemp("edges"))
    c = {"dir": d, "oi": {}, "ufi": {}, "idx": {}, "mapper": {}}
    for name, store in (("se", el.se_store()), ("rescue", el.rescue_store()), ("gate", el.gate_store())):
        fa = os.path.join(d, name + ".fa")
        synth.write_fasta(fa, store)
        c["oi"][name] = ol.Index.build(fa, el.SLOTS)
        c["ufi"][name] = os.path.join(d, name + ".ufi")
        c["oi"][name].save(c["ufi"][name])
        c["idx"][name] = api.Index.open(c["ufi"][name]).upload(0)
        c["mapper"][name] = api.Mapper(c["idx"][name], device=0)
    c["fa"] = os.path.join(d, "se.fa")
    reads, tags = el.se_cases()
    c["se"] = {"reads": reads, "tags": tags, "batches": []}
    for L, idx in sorted(_by_length(reads).items()):  # one batch per read length: 100, 150, 151, 152, 250, 600, 1 024
        bases, offs = reads_to_arrays([reads[i] for i in idx])
        c["se"]["batches"].append((L, idx, bases, offs))
    assert [b[0] for b in c["se"]["batches"]] == list(el.SWEEP_LENS)
    greads, _ = el.gate_cases()
    c["gate"] = reads_to_arrays(greads) + c["oi"]["gate"].map_se(*reads_to_arrays(greads), threads=4)
    yield c
    for m in c["mapper"].values():
        m.close()
    for idx in c["idx"].values():
        idx.close()


def _se_oracle(c, oi, method=6):
    """the oracle's results per batch of the single-end list (kept per method)"""
    key = ("ores", method)
    if key not in c["se"]:
        c["se"][key] = [oi.map_se(bases, offs, method=method, threads=4) for _, _, bases, offs in c["se"]["batches"]]
    return c["se"][key]


def _run_se(c, m, oi, method=6, stats=True):
    out = []
    for (L, idx, bases, offs), (ores, opaths, _) in zip(c["se"]["batches"], _se_oracle(c, oi, method)):
        gres, gops = m.map_se(bases, offs)
        compare_results(gres, gops, ores, opaths)
        if stats:
            out.append((L, m.dp_stats(), m.phase3()[1]))
    return out


def _run_gate(c, m):
    """the reads with a second, worse locus at an edge (edges_lib.gate_cases) -> dp_stats() of the call"""
    bases, offs, ores, opaths, cnt = c["gate"]
    assert cnt["n_ahsp_capped"] == 2 * len(ores)  # the oracle's AlignHSP turned two HSPs of every read away at its first test
    gres, gops = m.map_se(bases, offs)
    compare_results(gres, gops, ores, opaths)
    return len(ores)


# ---------------------------------------------------------------------------------------------------------------------------
# single-end: the full list on each road
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"URMAPX_INLINE_PHASE6": "1"}, {"URMAPX_NO_K2": "1"}], ids=["default", "inline_phase6", "no_k2"])
def test_se_edges_match_oracle(edges, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if "URMAPX_INLINE_PHASE6" in env:
        # a context of its own: one that has never run phase 6 as launches has no job array at all, and says so -- the knob took
        # effect, no read was parked (dp_stats() of a context that has parked before keeps showing its last parked call)
        ms = {k: api.Mapper(edges["idx"][k], device=0) for k in ("se", "gate")}
        _run_se(edges, ms["se"], edges["oi"]["se"], stats=False)
        _run_gate(edges, ms["gate"])
        for m in ms.values():
            with pytest.raises(api.UrmapxError):
                m.dp_stats()
            m.close()
        return
    stats = _run_se(edges, edges["mapper"]["se"], edges["oi"]["se"])
    print(stats)
    n = _run_gate(edges, edges["mapper"]["gate"])
    if not env:
        # phase 6 as launches of its own: reads parked with their HSPs as jobs.  Phase 3 aligns an HSP of more than 60 % of the read
        # inside the search kernel, so it is the 100-base batch (edits 22 bases from the end leave 77) that parks by the hundred.
        # No job is gated before its DP on this repeat-free store (every read has one locus: no hit lowers the cap under another
        # HSP's own penalty); the gate list is there for that.
        for L, st, _ in stats:
            assert st[0] >= st[1] > 0 and st[2] > 0 and st[3] == 0, (L, st)
        assert stats[0][1][1] > 300, stats
        # the gate list: every read parked with four jobs; the first round (jobs 0 and 1: the interior locus) makes the hit, the
        # cap it leaves gates both jobs of the copy at the edge before their DP
        st = edges["mapper"]["gate"].dp_stats()
        print("gate", st)
        assert st[0] == 4 * n and st[1] == n and st[2] > 0 and st[3] == 2 * n, st


@pytest.mark.parametrize("knob", ["URMAPX_PARK_PHASE3", "URMAPX_NO_CHAIN_ROWS"])
def test_se_edges_on_an_index_uploaded_another_way(edges, monkeypatch, knob):
    """phase 3 parked (the knob is read at upload -- the row layout stays -- and at every call), and the chain walk instead of the
    row layout (read at upload): an index of its own each"""
    monkeypatch.setenv(knob, "1")
    idx = api.Index.open(edges["ufi"]["se"]).upload(0)
    assert (idx.chain_row_bytes() == 0) == (knob == "URMAPX_NO_CHAIN_ROWS")
    m = api.Mapper(idx, device=0)
    stats = _run_se(edges, m, edges["oi"]["se"])
    print(stats)
    if knob == "URMAPX_PARK_PHASE3":
        # reads did park at phase 3, one DpJob each at least: nearly every read that is not a full-length hit, since an edit at most 22
        # bases from the end leaves an HSP of more than 60 % of the read (the 600- and 1 024-base instances do not park phase 3)
        assert all(p3[0] >= p3[1] > 1000 for L, _, p3 in stats if L <= 250), stats
    m.close()
    idx.close()


def test_se_edges_method7_on_a_maxix3_index(edges, tmp_path):
    """-veryfast: band radius 8, so a flank needs 16 bases beside it where method 6 needs 24 -- the oracle's outcome, compared as such"""
    oi = ol.Index.build(edges["fa"], el.SLOTS, max_ix=3)
    ufi = os.path.join(tmp_path, "vf.ufi")
    oi.save(ufi)
    o6 = np.concatenate([r[0]["dbpos"] for r in _se_oracle(edges, edges["oi"]["se"])])
    o7 = np.concatenate([r[0]["dbpos"] for r in _se_oracle(edges, oi, method=7)])
    assert ((o6 == el.UNMAPPED) & (o7 != el.UNMAPPED)).sum() > 500  # the flips moved
    idx = api.Index.open(ufi).upload(0)
    m = api.Mapper(idx, device=0, method=7)
    _run_se(edges, m, oi, method=7)
    m.close()
    idx.close()


def test_long_reads_at_the_edges_go_through_the_general_kernel(edges, monkeypatch):
    reads, _ = el.long_cases()
    bases, offs = reads_to_arrays(reads)
    ores, opaths, _ = edges["oi"]["se"].map_se(bases, offs, threads=4)
    m = edges["mapper"]["se"]
    monkeypatch.setenv("URMAPX_TEST_NO_GENERAL", "1")
    flagged, _ = m.map_se(bases, offs, allow_unsupported=True)
    assert (flagged["status"] != 0).all()  # none of them is the fast kernels'
    monkeypatch.delenv("URMAPX_TEST_NO_GENERAL")
    g, gops = m.map_se(bases, offs)
    compare_results(g, gops, ores, opaths)


# ---------------------------------------------------------------------------------------------------------------------------
# pairs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair_lists(edges):
    out = []
    for name, fn, which in (("pe_edge", el.pe_edge_cases, "se"), ("rescue", el.rescue_cases, "rescue")):
        reads, tags = fn()
        for L, idx in sorted(_by_length(reads, pairs=True).items()):
            sub = [r for i in idx for r in reads[2 * i:2 * i + 2]]
            bases, offs = reads_to_arrays(sub)
            out.append({"name": f"{name}{L}", "which": which, "reads": sub, "bases": bases, "offs": offs, "oracle": {}})
    assert [p["name"] for p in out] == ["pe_edge150", "rescue150", "rescue279"]
    return out


def _compare_pairs(g, gops, ores, opaths):
    """compare_results for pairs: every field it compares but exit_phase, which Search4 does not have -- the oracle leaves 0
    there, the pair kernels write whether the seed loop settled the pair"""
    assert (g["status"] == 0).all(), np.unique(g["status"])
    for name in ("dbpos", "seq_index", "coord", "score", "second", "mapq", "hit_count"):
        a, b = g[name].astype(np.int64), ores[name].astype(np.int64)
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, f"{name}: {len(bad)} mismatches, first mate {bad[0]}: gpu {a[bad[0]]} oracle {b[bad[0]]}"
    mapped = ores["dbpos"] != el.UNMAPPED
    assert (g["plus"][mapped] == ores["plus"][mapped]).all()
    for i in np.nonzero(mapped)[0]:
        o = int(g["path_off"][i])
        assert api.decode_path(gops[o:o + int(g["path_nops"][i])]) == opaths[i], f"mate {i}"


@pytest.mark.parametrize("road", ["default", "general", "veryfast"])
def test_pairs_at_the_edges_match_oracle(edges, pair_lists, monkeypatch, road):
    if road == "general":
        monkeypatch.setenv("URMAPX_TEST_PE_GENERAL", "1")
    vf = road == "veryfast"
    total = {}
    for p in pair_lists:
        if vf not in p["oracle"]:
            p["oracle"][vf] = edges["oi"][p["which"]].map_pe(p["bases"], p["offs"], threads=4, veryfast=vf)
        ores, opaths, cnt = p["oracle"][vf]
        for k, v in cnt.items():
            total[k] = total.get(k, 0) + v
        m = api.Mapper(edges["idx"][p["which"]], device=0)
        m.set_pe_veryfast(vf)
        g, gops = m.map_pe(p["bases"], p["offs"])
        _compare_pairs(g, gops, ores, opaths)
        m.close()
    if not vf:  # the batch does what it was built for (Search5 has no ScanPair)
        for k in ("n_scan_vit", "n_scan_hits", "n_scan_low", "n_scan_pad", "n_tail_bytes"):
            assert total[k] >= 20, (k, total[k])


def test_pair_records_at_the_edges(edges, pair_lists, tmp_path):
    """with set_pair_info: the per-pair records (each mate's top hit before SetMappedPos, the second pair), compared through
    -tabbedout's line per pair as the oracle writes it"""
    for p in pair_lists:
        sub = el.strip_mate_suffix(p["reads"])
        f1, f2, tab = (os.path.join(tmp_path, p["name"] + x) for x in ("_1.fq", "_2.fq", ".tab"))
        synth.write_fastq(f1, sub[0::2])
        synth.write_fastq(f2, sub[1::2])
        edges["oi"][p["which"]].map_file_pe_tab(f1, f2, os.path.join(tmp_path, "o.sam"), tab, threads=4)
        idx = edges["idx"][p["which"]]
        m = api.Mapper(idx, device=0)
        m.set_pair_info(True)
        labels, bases, offs, quals = api.interleave_pairs(api.read_fastq_arrays(f1), api.read_fastq_arrays(f2))
        res, ops = m.map_pe(bases, offs)
        assert (res["status"] == 0).all()
        info = m.pair_info(len(res) // 2)
        assert idx.tab_pe(res, info, labels, offs, sam_on=True) == open(tab, "rb").read(), p["name"]
        assert idx.sam_header_sq() + idx.sam_pe(res, ops, labels, bases, offs, quals) == open(os.path.join(tmp_path, "o.sam"), "rb").read()
        m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# text and file roads on the golden fixtures (the reference binary's own bytes)
# ---------------------------------------------------------------------------------------------------------------------------
def _gold(name, tmp_path=None):
    with gzip.open(os.path.join(GOLD, name + ".gz"), "rb") as z:
        data = z.read()
    if tmp_path is None:
        return data
    p = os.path.join(tmp_path, name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def _records(data, drop=b"@PG"):
    return [l for l in data.split(b"\n") if l and not l.startswith(drop)]


@pytest.fixture(scope="module")
def gold_ufis(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("edges_gold"))
    out = {}
    for name in ("edges", "edges_rescue"):
        out[name] = os.path.join(d, name + ".ufi")
        ol.Index.build(os.path.join(GOLD, name + ".fa"), el.SLOTS).save(out[name])
    return out


def test_text_roads_give_the_golden_sam(gold_ufis):
    idx = api.Index.open(gold_ufis["edges"]).upload(0)
    m = api.Mapper(idx, device=0)
    sam, rep = m.map_text_se(_gold("edges_se.fq"))
    want = _records(_gold("edges_se.sam"), b"@")
    assert rep["reason"] == api.TEXT_OK and rep["records"] == len(want), rep
    assert _records(sam, b"@") == want
    m.close()
    idx.close()
    idx = api.Index.open(gold_ufis["edges_rescue"]).upload(0)
    m = api.Mapper(idx, device=0)
    sam, rep = m.map_text_pe(_gold("edges_pe_1.fq"), _gold("edges_pe_2.fq"))
    want = _records(_gold("edges_pe.sam"), b"@")
    assert rep["reason"] == api.TEXT_OK and rep["records"] == len(want), rep
    assert _records(sam, b"@") == want
    m.close()
    idx.close()


def _run(args):
    r = subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]


def test_cli_file_to_file_gives_the_golden_sam_and_bam(gold_ufis, tmp_path):
    """`urmap -map` / `-map2` file to file: the golden SAM bytes; -bamout carries the same fields -- among them a record at a
    sequence's first base (pos 0) and one ending at its last base with their reg2bin (bam_lib.read_bam checks every record's bin),
    and unplaced mates"""
    se, p1, p2 = (_gold(n, tmp_path) for n in ("edges_se.fq", "edges_pe_1.fq", "edges_pe_2.fq"))
    sam, bam = os.path.join(tmp_path, "o.sam"), os.path.join(tmp_path, "o.bam")
    lens = dict(zip((f"edge{i + 1}" for i in range(5)), el.SE_LENGTHS))
    for args, ufi, gold, paired in ((["-map", se], gold_ufis["edges"], "edges_se.sam", False),
                                    (["-map2", p1, "-reverse", p2], gold_ufis["edges_rescue"], "edges_pe.sam", True)):
        _run(args + ["-ufi", ufi, "-samout", sam, "-quiet"])
        text = open(sam, "rb").read()
        assert _records(text) == _records(_gold(gold))
        _run(args + ["-ufi", ufi, "-bamout", bam, "-quiet"])
        _, refs, lines = bl.read_bam(bl.inflate(open(bam, "rb").read()))
        assert refs == bl.refs_of_header(bl.sam_header(text)) and lines == bl.sam_records(text)
        f = [l.split("\t") for l in lines]
        if not paired:
            assert sum(1 for x in f if x[3] == "1" and x[5] == "150M") >= 10  # first base of a sequence
            assert sum(1 for x in f if x[5] == "150M" and int(x[3]) - 1 + 150 == lens[x[2]]) >= 10  # last base of a sequence
        else:
            assert sum(1 for x in f if int(x[1]) & 4 and not int(x[1]) & 8) >= 10  # an unplaced mate beside a placed one
            assert sum(1 for x in f if x[3] == "1") >= 2
