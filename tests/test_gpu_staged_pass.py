"""GPU: the staged pass behaves alike for every caller (bam_sort_dev.h: cut_chunks, staged_pass, staged_alone; Beside).  One input --
short reads, adjacent mates of which some are duplicates, and one record longer than any small staging buffer and than a BGZF member --
goes through urmapx_bam_depth, urmapx_bam_stats and urmapx_bam_pileup with staged chunks of one record, of 4096 bytes and of
everything, and through urmapx_bam_sort_with with all three taken on the way, in core and on the external road, without and with
marking.  Every result is its host twin's, which is first held against the numpy models on the CPU, and every count of staged chunks
is that of bam_sort.h's chunk_end over the records' lengths (chunk_starts of test_gpu_bam_sort_external.py)."""
import numpy as np
import pytest

import bam_lib as bl
import bam_sort_lib as sl
import depth_lib as dl
import pileup_lib as pl
import stats_lib as stl
from stats_lib import rec
from test_gpu_bam_sort_external import chunk_starts, lengths
from test_pileup_cpu import ANY

pytestmark = pytest.mark.gpu

KNOBS = ("URMAPX_TEST_SORT_STAGE", "URMAPX_TEST_SORT_PARTITION", "URMAPX_TEST_SORT_SLICE")
NAMES, LENS = ["one", "two"], [5000, 5000]
LONG = 70000  # bases of the long record: more than 65 280, a member, and than any stage asked for here but the largest
STAGES = (1, 4096, 1 << 30)


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def make_input():
    """-> (records, seqs): some 300 records in no order on two references of 5 000 bases"""
    rng = np.random.default_rng(11)
    seqs = [rng.choice(list(b"ACGT"), l).astype(np.uint8).tobytes() for l in LENS]
    bases = lambda l: rng.choice([1, 2, 4, 8, 15], l, p=[0.24, 0.24, 0.24, 0.24, 0.04])  # noqa: E731
    quals = lambda l: bytes(rng.integers(2, 42, l).astype(np.uint8))  # noqa: E731
    recs = []
    for k in range(70):  # adjacent mates at 14 places, five pairs at each: four of five are duplicates
        ref, at, l = k % 2, 100 + 330 * (k % 14), 30 + 9 * (k % 14)  # (a place's pairs are as long: the reverse mates end alike)
        common = dict(ref=ref, next_ref=ref, mapq=int(rng.integers(0, 61)), cigar="%dM" % l, name=b"p%d" % k)
        recs.append(rec(flag=0x63, pos=at, next_pos=at + 200, tlen=200 + l, seq=bases(l), qual=quals(l), **common))
        recs.append(rec(flag=0x93, pos=at + 200, next_pos=at, tlen=-(200 + l), seq=bases(l), qual=quals(l), **common))
    for k in range(160):  # lone reads of every kind, with clips, insertions and deletions, some beyond the reference's end
        l = int(rng.integers(30, 151))
        cigar = ["%dM" % l, "5S%dM" % (l - 5), "%dM2I%dM" % (10, l - 12), "%dM3D%dM" % (l - 8, 8)][k % 4]
        flag = int(rng.choice([0, 0x10, 0x400, 0x100, 0x800, 0x200]))
        recs.append(rec(flag=flag, ref=int(rng.integers(0, 2)), pos=int(rng.integers(0, 4990)), mapq=int(rng.integers(0, 61)), cigar=cigar, seq=bases(l), qual=quals(l),
                        name=b"f%d" % k))
    recs += [rec(flag=0x4, seq=bases(40), name=b"u%d" % k) for k in range(5)]
    recs.insert(150, rec(ref=1, pos=100, mapq=30, cigar="%dM" % LONG, seq=bases(LONG), qual=quals(LONG), name=b"long"))
    return b"".join(recs), seqs


@pytest.fixture(scope="module")
def case():
    """the input, and what the host twins make of it -- each held against its model before anything goes to the device"""
    from urmap_amd import api
    records, seqs = make_input()
    lens = lengths(records)
    assert 290 <= len(lens) <= 320 and max(lens) > LONG > sl.MEMBER
    host = {"depth": api.bam_depth_host(records, 2, NAMES, LENS), "stats": api.bam_stats_host(records, 2, NAMES, LENS),
            "pileup": api.bam_pileup_host(records, 2, NAMES, LENS, seqs, opts=ANY)}
    assert host["depth"] == dl.model(records, NAMES, LENS)
    assert host["stats"] == stl.model(records, NAMES, LENS)
    assert host["pileup"] == pl.model(records, NAMES, LENS, seqs, ANY)
    assert len(pl.parse(host["pileup"])["sites"]) > 100
    sort = {}
    for markdup in (False, True):
        out = api.bam_sort_host(records, 2, markdup=markdup, report=True, **beside(seqs))
        stream = bl.inflate(out[0])
        assert out[2] == dl.model(stream, NAMES, LENS) and out[3] == stl.model(stream, NAMES, LENS) and out[4] == pl.model(stream, NAMES, LENS, seqs, ANY)
        assert not markdup or out[5]["pairs_duplicate"] == 56
        sort[markdup] = seen(out)
    return {"records": records, "seqs": seqs, "lens": lens, "host": host, "sort": sort}


def beside(seqs):
    return dict(depth=(NAMES, LENS), stats=(NAMES, LENS), pileup=(NAMES, LENS, seqs, ANY))


def seen(out):
    """of bam_sort's result: the stream, the index in places of the stream (the members' sizes are the compressor's), the three texts"""
    from urmap_amd import api
    members, bai = out[:2]
    table = sl.member_places(sl.BgzfFile(members + api.BGZF_EOF), 0)
    return (bl.inflate(members), sl.index_in_places(sl.parse_bai(bai), table)) + tuple(out[2:5])


@pytest.mark.parametrize("stage", STAGES)
def test_on_its_own_every_by_product_is_its_host_twin_in_the_same_chunks(monkeypatch, case, stage):
    from urmap_amd import api
    monkeypatch.setenv("URMAPX_TEST_SORT_STAGE", str(stage))
    records, seqs = case["records"], case["seqs"]
    want_chunks = len(chunk_starts(case["lens"], stage))
    assert want_chunks == {1: len(case["lens"]), 4096: want_chunks, 1 << 30: 1}[stage] and (stage != 4096 or 10 < want_chunks < len(case["lens"]))
    *depth, drep = api.bam_depth(records, 2, NAMES, LENS, device=0, report=True)
    stats, srep = api.bam_stats(records, 2, NAMES, LENS, device=0, report=True)
    vcf, prep = api.bam_pileup(records, 2, NAMES, LENS, seqs, opts=ANY, device=0, report=True)
    assert tuple(depth) == case["host"]["depth"]
    assert stats == case["host"]["stats"]
    assert vcf == case["host"]["pileup"]
    assert [drep["stage_chunks"], srep["stage_chunks"], prep["stage_chunks"]] == [want_chunks] * 3


ROADS = {"as it is": {}, "partitions of a slice, chunks of 4096 bytes": {"URMAPX_TEST_SORT_PARTITION": "1", "URMAPX_TEST_SORT_STAGE": "4096", "URMAPX_TEST_SORT_SLICE": "1"},
         "partitions of a slice, chunks of a record": {"URMAPX_TEST_SORT_PARTITION": "1", "URMAPX_TEST_SORT_STAGE": "1", "URMAPX_TEST_SORT_SLICE": "1"}}


@pytest.mark.parametrize("road", list(ROADS))
@pytest.mark.parametrize("markdup", [False, True])
def test_beside_the_sort_all_three_are_the_host_sorts_on_every_road(monkeypatch, case, markdup, road):
    from urmap_amd import api
    for k, v in ROADS[road].items():
        monkeypatch.setenv(k, v)
    out = api.bam_sort(case["records"], 2, device=0, budget=0, markdup=markdup, report=True, **beside(case["seqs"]))
    got, want = seen(out), case["sort"][markdup]
    for k, what in enumerate(("the stream", "the index", "the depth", "the statistics", "the pileup")):
        assert got[k] == want[k], what
    rep = out[5]
    if ROADS[road]:
        stage = int(ROADS[road]["URMAPX_TEST_SORT_STAGE"])
        assert rep["external"] == 1 and rep["partitions"] == -(-len(case["records"]) // sl.MEMBER) >= 3
        assert rep["stage_chunks"] == len(chunk_starts(case["lens"], stage, look=markdup))
    else:
        assert rep["external"] == 0 and rep["stage_chunks"] == 0
