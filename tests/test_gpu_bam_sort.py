"""GPU tests of -sort: the device sort of BAM records (bam_sort.hip) against the host function and against the yardstick of
tests/bam_sort_lib.py -- record counts at the edges of a wavefront, of a workgroup's tile and of a whole grid, stability, the digits the
keys need, the gather's shapes, the slices --, and `urmap ... -bamout out.bam -sort` through its roads."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_lib as bl
import bam_sort_lib as sl
from test_bam_sort_cpu import check_sorted_file

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "urmap_amd", "urmap")

TILE = 1024          # bam_sort.hip: records a workgroup of the scatter kernel takes at the least
MAX_BLOCKS = 512     # workgroups of a sort pass: beyond MAX_BLOCKS * TILE records a workgroup walks several tiles

TINY = np.dtype([("block_size", "<u4"), ("ref", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cigar", "<u2"),
                 ("flag", "<u2"), ("l_seq", "<u4"), ("next_ref", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"), ("name", "S2")])
assert TINY.itemsize == 38


def tiny_records(ref, pos):
    """38-byte records (a one-letter name, no CIGAR, no bases), record i carrying i in tlen so that the order they come out in shows"""
    ref, pos = np.asarray(ref, np.int64), np.asarray(pos, np.int64)
    a = np.zeros(len(ref), TINY)
    a["block_size"], a["ref"], a["pos"], a["l_name"], a["name"] = 34, ref, pos, 2, b"a"
    a["bin"] = np.where(ref < 0, 4680, (4681 + (pos >> 14)) & 0xFFFF)
    a["flag"] = np.where(ref < 0, 4, 0)
    a["next_ref"], a["next_pos"], a["tlen"] = -1, -1, np.arange(len(ref))
    return a.tobytes()


def stable_order(ref, pos):
    """the order the sort must give: refID as unsigned, then pos as unsigned, ties in input order (lexsort is stable)"""
    return np.lexsort((np.asarray(pos, np.int64) & 0xFFFFFFFF, np.asarray(ref, np.int64) & 0xFFFFFFFF))


def passes_needed(n_ref, pos):
    """histogram-scan-scatter rounds of 8 bits: the references 0 .. n_ref (the last for "none"), the positions 0 .. largest + 1 (likewise)"""
    placed = [int(p) for p in pos if p >= 0]
    bits = max(1, int(n_ref).bit_length()) + max(1, (max(placed, default=0) + 1).bit_length())
    return (bits + 7) // 8


def both(records, n_ref, in_front=0):
    """the device sort and the host sort of the same records: the same inflated stream, the same index in places of the stream"""
    from urmap_amd import api
    dm, dbai, drep = api.bam_sort(records, n_ref, device=0, bytes_in_front=in_front, report=True)
    hm, hbai, hrep = api.bam_sort_host(records, n_ref, bytes_in_front=in_front, report=True)
    stream = bl.inflate(dm)
    assert stream == bl.inflate(hm), "the device's stream differs from the host's"
    for k in ("stream_bytes", "records", "no_coor"):
        assert drep[k] == hrep[k], k
    fd, fh = sl.BgzfFile(b"\0" * in_front + dm + api.BGZF_EOF), sl.BgzfFile(b"\0" * in_front + hm + api.BGZF_EOF)
    db, hb = sl.parse_bai(dbai), sl.parse_bai(hbai)
    td = sl.member_places(fd, in_front)
    assert sl.index_in_places(db, td) == sl.index_in_places(hb, sl.member_places(fh, in_front)), "the device's index differs from the host's"
    sizes = [s for _, s in fd.members(in_front)][:-1]
    assert all(s == sl.MEMBER for s in sizes[:-1]) and (not sizes or 0 < sizes[-1] <= sl.MEMBER)
    return stream, db, fd, td, drep


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE + 1, MAX_BLOCKS * TILE + 1])
def test_device_equals_host_at_the_edges_of_the_grid(n):
    rng = np.random.default_rng(n)
    n_ref = 300
    ref = rng.integers(-1, n_ref, n)
    pos = np.where(ref < 0, -1, rng.integers(0, 1 << 20, n))
    stream, b, f, table, rep = both(tiny_records(ref, pos), n_ref)
    out = np.frombuffer(stream, TINY)
    assert (out["tlen"] == stable_order(ref, pos)).all()
    assert rep["sort_passes"] == (passes_needed(n_ref, pos) if n else 0)
    if n > TILE:
        assert rep["sort_passes"] == 4  # 9 bits of reference, 21 of position
    if 0 < n <= TILE + 1:
        sl.check_index(b, sl.split_records(stream), table, n_ref)


@pytest.mark.parametrize("keys", [1, 2])
def test_equal_keys_keep_their_input_order(keys):
    n = 1000
    pos = 777 + 1000 * (np.arange(n) % keys)[::-1]
    stream, *_ = both(tiny_records(np.zeros(n, int), pos), 1)
    out = np.frombuffer(stream, TINY)
    assert (out["tlen"] == stable_order(np.zeros(n, int), pos)).all()
    if keys == 1:
        assert (out["tlen"] == np.arange(n)).all()


@pytest.mark.parametrize("what", ["only_unmapped", "none_unmapped", "high_pos"])
def test_keys(what):
    n = 300
    rng = np.random.default_rng(5)
    if what == "only_unmapped":
        ref, pos, n_ref = np.full(n, -1), np.full(n, -1), 3
    elif what == "none_unmapped":
        ref, pos, n_ref = rng.integers(0, 3, n), rng.integers(0, 50000, n), 3
    else:  # a position that needs bit 30: beyond what the bins cover; the order and the stream hold, and the index of what lies below 2^29
        ref, pos, n_ref = rng.integers(0, 2, n), np.where(rng.integers(0, 2, n) == 1, (1 << 30) + 5, rng.integers(0, 1 << 20, n)), 2
    stream, b, f, table, rep = both(tiny_records(ref, pos), n_ref)
    out = np.frombuffer(stream, TINY)
    assert (out["tlen"] == stable_order(ref, pos)).all()
    assert b.n_no_coor == (n if what == "only_unmapped" else 0) == rep["no_coor"]
    sl.check_index(b, sl.split_records(stream), table, n_ref)
    if what == "high_pos":
        assert rep["sort_passes"] == 5  # 2 bits of reference, 31 of position
        assert all(0 < len(r["linear"]) <= (1 << 20) >> 14 for r in b.refs)  # (no window for the records beyond)


@pytest.mark.parametrize("n_ref", [1, 255, 256, 257])
def test_the_digit_count_follows_n_ref(n_ref):
    n = 2000
    rng = np.random.default_rng(n_ref)
    ref = np.concatenate([rng.integers(-1, n_ref, n - 3), [n_ref - 1, 0, -1]])
    pos = np.where(ref < 0, -1, np.concatenate([rng.integers(0, 201, n - 3), [200, 0, 0]]))
    stream, b, f, table, rep = both(tiny_records(ref, pos), n_ref)
    assert (np.frombuffer(stream, TINY)["tlen"] == stable_order(ref, pos)).all()
    bits = n_ref.bit_length() + 8  # values 0 .. n_ref (the last for "no reference"), positions 0 .. 201 (the last for "no position")
    assert rep["sort_passes"] == (bits + 7) // 8 == {1: 2, 255: 2, 256: 3, 257: 3}[n_ref]
    sl.check_index(b, sl.split_records(stream), table, n_ref)


def test_gather_shapes():
    """the shortest records, one longer than a member, names of every length mod 4 so that records start at every address residue, a
    CIGAR of more than 15 ops -- all in one input, whose sorted stream the long record crosses two cuts of"""
    refs = [("a", 300000), ("b", 300000)]
    rng = np.random.default_rng(11)
    lines = []
    for i in range(400):
        name = "n" * (1 + i % 9)
        p = int(rng.integers(1, 200000))
        if i % 50 == 7:
            cigar, q = "".join("3M1I" if k % 2 else "3M1D" for k in range(20)) + "5M", 3 * 20 + 10 + 5
        else:
            cigar, q = "%dM" % (30 + i % 5), 30 + i % 5
        lines.append(f"{name}\t0\t{refs[i % 2][0]}\t{p}\t9\t{cigar}\t*\t0\t0\t{'ACGT'[i % 4] * q}\t{'F' * q}")
    lines.insert(123, "long\t0\ta\t100000\t9\t70000M\t*\t0\t0\t%s\t%s" % ("C" * 70000, "G" * 70000))
    lines.insert(300, "u\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*")
    records = bl.sam_to_bam_records("\n".join(lines) + "\n", refs) + tiny_records([0, -1, 1], [5, -1, 299999])
    assert max(len(r) for _, r in sl.split_records(records)) > sl.MEMBER + 36
    starts = set(o % 4 for o, _ in sl.split_records(records))
    stream, b, f, table, rep = both(records, 2, in_front=1234)
    _, recs = sl.check_stream(f.blob[1234:-28], records)
    assert starts == {0, 1, 2, 3} == set(o % 4 for o, _ in recs)
    sl.check_index(b, recs, table, 2)
    sl.check_queries(b, f, [r for _, r in recs], [(0, 0, 10), (0, 99999, 100000), (0, 169998, 169999), (0, 169999, 170001), (1, 299999, 300000), (1, 0, 300000)])


@pytest.mark.parametrize("members", [1, 3])
def test_slices(monkeypatch, members):
    """a small input made in several slices: the same inflated bytes and the same index as in one slice; records straddle slice ends"""
    rng = np.random.default_rng(3)
    lines = [f"r{i}\t0\tc\t{int(rng.integers(1, 900000))}\t1\t{40 + i % 7}M\t*\t0\t0\t{'A' * (40 + i % 7)}\t{'#' * (40 + i % 7)}" for i in range(4000)]
    records = bl.sam_to_bam_records("\n".join(lines) + "\n", [("c", 1000000)])
    whole = both(records, 1)
    assert whole[4]["slices"] == 1 and len(records) > 6 * sl.MEMBER
    monkeypatch.setenv("URMAPX_TEST_SORT_SLICE", str(members))
    sliced = both(records, 1)
    from urmap_amd import api
    offs = [o for o, _ in sl.split_records(records)]
    assert api.bam_sort(records, 1, starts=offs[::501])[1] == api.bam_sort(records, 1)[1]  # (the walk from known record starts: the same index)
    assert sliced[4]["slices"] == -(-len(records) // (members * sl.MEMBER)) > 1
    assert sliced[0] == whole[0]
    assert sl.index_in_places(sliced[1], sliced[3]) == sl.index_in_places(whole[1], whole[3])
    cuts = [k * members * sl.MEMBER for k in range(1, sliced[4]["slices"])]
    recs = sl.split_records(whole[0])
    assert all(any(o < c < o + len(r) for o, r in recs) for c in cuts), "no record straddles a slice's end"


# ---- the golden inputs: device against host, and the command line ----
def gold(name):
    return open(os.path.join(GOLD, name), "rb").read()


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    d = tmp_path_factory.mktemp("bamsort")
    out = {"dir": str(d)}
    for name in ("g", "r"):
        out[name] = os.path.join(d, name + ".ufi")
        with gzip.open(os.path.join(GOLD, name + ".ufi.gz"), "rb") as z, open(out[name], "wb") as f:
            f.write(z.read())
    return out


@pytest.mark.parametrize("names,ufi", [(("se150.fq",), "g"), (("pe120_rep_1.fq", "pe120_rep_2.fq"), "r")])
def test_device_against_host_on_the_golden_inputs(golden, names, ufi):
    from urmap_amd import api
    idx = api.Index.open(golden[ufi]).upload(0)
    m = api.Mapper(idx, device=0)
    try:
        m.set_bam(True)
        raw, rep = m.map_text_se(gold(names[0])) if len(names) == 1 else m.map_text_pe(gold(names[0]), gold(names[1]))
        assert rep["reason"] == api.TEXT_OK
    finally:
        m.close()
    n_ref = len(idx.directory())
    stream, b, f, table, _ = both(raw, n_ref, in_front=777)
    _, recs = sl.check_stream(f.blob[777:-28], raw)
    sl.check_index(b, recs, table, n_ref)
    lengths = [l for _, l, _ in idx.directory()]
    sl.check_queries(b, f, [r for _, r in recs], sl.edge_regions(lengths, np.random.default_rng(1), 60))


def _run(args, ok=True, **kw):
    r = subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)
    if ok:
        assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def _se(golden):
    return ["-map", os.path.join(GOLD, "se150.fq"), "-ufi", golden["g"], "-quiet"]


def _pe(golden):
    return ["-map2", os.path.join(GOLD, "pe150_1.fq"), "-reverse", os.path.join(GOLD, "pe150_2.fq"), "-ufi", golden["g"], "-quiet"]


@pytest.mark.parametrize("kind", ["se", "pe"])
def test_cli(golden, kind):
    args = _se(golden) if kind == "se" else _pe(golden)
    plain, out = (os.path.join(golden["dir"], f"{kind}_{n}.bam") for n in ("plain", "sorted"))
    _run(args + ["-bamout", plain])
    assert not os.path.exists(plain + ".bai")  # (that file's bytes are pinned by tests/test_gpu_bam.py, which this flag leaves alone)
    _run(args + ["-bamout", out, "-sort"])
    inflated, b, f, recs, refs = check_sorted_file(open(out, "rb").read(), open(out + ".bai", "rb").read(), open(plain, "rb").read())
    assert len(recs) >= 400 and b.n_no_coor == sum(1 for _, r in recs if sl.fields(r)[0] < 0)
    sl.check_queries(b, f, [r for _, r in recs], sl.edge_regions([L for _, L in refs], np.random.default_rng(2), 60))
    r = _run(args[:-1] + ["-bamout", out, "-sort"])
    assert b"Seconds to sort" in r.stderr
    if kind == "pe":
        return
    # the same inflated records whatever the road (the @PG line differs: it holds the command line)
    def records_of(path):
        data = bl.inflate(open(path, "rb").read())
        text, refs2, _ = bl.read_bam(data)
        return data[len(bl.bam_header(text, refs2)):]
    want = records_of(out)
    for extra, env in ((["-streams", "1"], {}), (["-batch", "64"], {}), (["-host"], {}), (["-threads", "3"], {"URMAPX_HOST_TEXT": "1"})):
        other = os.path.join(golden["dir"], "other.bam")
        _run(args + ["-bamout", other, "-sort"] + extra, env={**os.environ, **env})
        assert records_of(other) == want, extra
        check_sorted_file(open(other, "rb").read(), open(other + ".bai", "rb").read(), open(plain, "rb").read())


def test_cli_refusals(golden):
    out = os.path.join(golden["dir"], "no.bam")
    sam = os.path.join(golden["dir"], "no.sam")
    for args, word in ((["-samout", sam, "-sort"], b"-bamout"), (["-bamout", out, "-sort", "-samshards", "2"], b"-samshards"),
                       (["-bamout", "/dev/stdout", "-sort"], b"pipe")):
        r = _run(_se(golden) + args, ok=False)
        assert r.returncode != 0 and b"-sort" in r.stderr and word in r.stderr and len(r.stderr.strip().split(b"\n")) == 2, r.stderr  # ("---Fatal error---" and one line)
        assert r.stdout == b"" and not os.path.exists(out) and not os.path.exists(out + ".bai") and not os.path.exists(sam)
    r = subprocess.run(f"'{EXE}' -map '{os.path.join(GOLD, 'se150.fq')}' -ufi '{golden['g']}' -quiet -bamout /dev/stdout -sort | cat", shell=True,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.stdout == b"" and b"-sort" in r.stderr
