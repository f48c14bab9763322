"""GPU tests of -bgzf: the device deflate kernel (bgzf_gpu.hip) on its edge shapes, what it must achieve against the text's order-0
entropy, the text stage with urmapx_text_set_bgzf, and `urmap -map / -map2 ... -bgzf` through every output road.  Every byte string
goes through the walker of tests/test_bgzf_cpu.py (magic, BC field, BSIZE chain, per-member inflate, CRC-32, ISIZE, end marker)."""
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

from test_bgzf_cpu import EOF_MEMBER, PIECE, check_pieces, seeded_bytes, walk_bgzf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "urmap_amd", "urmap")


def gold(name):
    return open(os.path.join(GOLD, name), "rb").read()


def roundtrip(data):
    from urmap_amd import api
    z = api.bgzf_compress(data, device=0)
    members = walk_bgzf(z)
    check_pieces(members, data)
    assert len(z) <= len(data) + 31 * len(members) + 28
    return z, members


def no_repeat_600():
    """600 bytes with all 256 values in which no pair of neighbours occurs twice (so no three bytes do): 0..255 by steps of 1, then
    of 3, then of 5"""
    b = bytes(list(range(256)) + [(3 * i) % 256 for i in range(256)] + [(5 * i) % 256 for i in range(88)])
    pairs = [b[i:i + 2] for i in range(len(b) - 1)]
    assert len(b) == 600 and len(set(b)) == 256 and len(set(pairs)) == len(pairs)
    return b


EDGE = {
    "empty": b"",
    "one_byte": b"x",
    "two_bytes": b"xy",
    "run_of_A": b"A" * PIECE,
    "no_repeat_600": None,
    "far_copy": None,
    "piece_minus_1": None, "piece": None, "piece_plus_1": None, "three_pieces_and_7": None,
    "window_edge": None, "window_edge_flushed": None,
}


def edge_input(name):
    sam = gold("se150.sam")
    rnd = seeded_bytes(40000, 11)
    if name == "no_repeat_600":
        return no_repeat_600()
    if name == "far_copy":  # the copy's source is 40 000 back: beyond the window, it must not be referenced
        return rnd + rnd[:30000]
    if name == "window_edge":
        # y's source is 32 769 back (one too many: it must come as literals), x's exactly 32 768 back (the largest distance).  Between them
        # a run, which enters one hash only: a matcher that keeps the latest position per hash still holds x's when the copy comes
        x, y = seeded_bytes(300, 12), seeded_bytes(300, 13)
        return y + b"A" + x + b"A" * (32768 - 300 - 300) + y + x
    if name == "window_edge_flushed":  # the same distances with random bytes between: they take every hash over several times
        a, b = seeded_bytes(32768, 12), seeded_bytes(1, 13)
        return a[:300] + a[300:] + a[:300] + seeded_bytes(32769 - 600, 14) + b + a[:300]
    reps = (sam * (4 * PIECE // len(sam) + 1))
    n = {"piece_minus_1": PIECE - 1, "piece": PIECE, "piece_plus_1": PIECE + 1, "three_pieces_and_7": 3 * PIECE + 7}.get(name)
    return reps[:n] if n else EDGE[name]


@pytest.mark.parametrize("name", list(EDGE))
def test_kernel_edge_shapes(name):
    data = edge_input(name)
    z, members = roundtrip(data)
    if name == "empty":
        assert z == EOF_MEMBER
    if name == "run_of_A":  # length-258 matches at distance 1: a few hundred bytes
        assert len(z) < 600 and members[0][1] == 2
    if name == "far_copy":
        assert all(m[1] == 0 for m in members)  # nothing within reach repeats: stored


def test_random_mebibyte_is_stored_in_every_member():
    data = seeded_bytes(1 << 20, 3)
    z, members = roundtrip(data)
    assert all(btype == 0 and size == len(text) + 31 for text, btype, size in members)


def test_golden_pairs_sam_and_two_runs_agree():
    from urmap_amd import api
    data = gold("pe150.sam")
    z, _ = roundtrip(data)
    assert api.bgzf_compress(data, device=0) == z
    assert api.bgzf_compress(data, device=0, eof=False) + EOF_MEMBER == z


def test_cap_below_bound_is_refused():
    from urmap_amd import api
    with pytest.raises(api.UrmapxError) as e:
        api.bgzf_compress(b"ACGT" * 100, device=0, cap=api.bgzf_bound(400) - 1)
    assert e.value.code == -5


# ---- ratio: bounds computed here from the input, none taken from the code under test ----
def entropy_bytes(piece):
    c = np.bincount(np.frombuffer(piece, dtype=np.uint8), minlength=256).astype(np.float64)
    c = c[c > 0]
    return float(-(c * np.log2(c / c.sum())).sum() / 8.0)


def pieces_of(data):
    return [data[o:o + PIECE] for o in range(0, len(data), PIECE)]


def zlib_level1(data):
    total = 0
    for p in pieces_of(data):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        total += len(c.compress(p) + c.flush()) + 26
    return total + 28


@pytest.mark.parametrize("name", ["se150.sam", "se250.sam", "pe100_noisy.sam"])
def test_ratio_golden_sam_text(name):
    from urmap_amd import api
    data = gold(name)
    ps = pieces_of(data)
    bound = 1.05 * sum(entropy_bytes(p) for p in ps) + 300 * len(ps)
    ref = zlib_level1(data)
    assert ref <= bound, (ref, bound)  # self-check: the bound is one a real deflate meets
    assert len(data) > bound           # ... and a stored-only output does not
    z = api.bgzf_compress(data, device=0)
    print(f"{name}: text {len(data)}, device {len(z)} ({len(z) / len(data):.3f}), zlib -1 {ref} ({ref / len(data):.3f}), bound {bound:.0f}")
    assert b"".join(m[0] for m in walk_bgzf(z)) == data
    assert len(z) <= bound, (len(z), bound)


def test_ratio_match_free_input_needs_dynamic_codes():
    from urmap_amd import api
    rng = np.random.default_rng(1)
    n = 200000
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]
    quals = rng.integers(33, 73, n).astype(np.uint8)
    data = np.where(rng.random(n) < 0.5, letters, quals).astype(np.uint8).tobytes()
    bound = 1.25 * entropy_bytes(data)
    ref = zlib_level1(data)
    assert ref <= bound, (ref, bound)
    z = api.bgzf_compress(data, device=0)
    print(f"match-free: text {len(data)}, device {len(z)} ({len(z) / entropy_bytes(data):.3f} x entropy), zlib -1 {ref / entropy_bytes(data):.3f} x")
    assert b"".join(m[0] for m in walk_bgzf(z)) == data
    assert len(z) <= bound, (len(z), bound)


# ---- text stage ----
@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    from urmap_amd import api
    d = tmp_path_factory.mktemp("bgzf")
    ufi = os.path.join(d, "g.ufi")
    with gzip.open(os.path.join(GOLD, "g.ufi.gz"), "rb") as z, open(ufi, "wb") as f:
        f.write(z.read())
    idx = api.Index.open(ufi).upload(0)
    m = api.Mapper(idx, device=0)
    yield {"index": idx, "mapper": m, "ufi": ufi, "dir": str(d)}
    m.close()


def test_text_stage_members_inflate_to_the_plain_text(golden):
    from urmap_amd import api
    m = golden["mapper"]
    se = gold("se150.fq")
    p1, p2 = gold("pe150_1.fq"), gold("pe150_2.fq")
    plain_se, _ = m.map_text_se(se)
    plain_pe, _ = m.map_text_pe(p1, p2)
    lines = se.split(b"\n")[:-1]
    chunks = [b"\n".join(lines[a:b]) + b"\n" for a, b in ((0, 4 * 120), (4 * 120, len(lines)))]
    plain_chunks = [m.map_text_se(c)[0] for c in chunks]
    m.set_bgzf(True)
    try:
        for got, want in ((m.map_text_se(se), plain_se), (m.map_text_pe(p1, p2), plain_pe)):
            z, rep = got
            assert rep["reason"] == api.TEXT_OK, rep
            assert rep["sam_bytes"] == len(z) and rep["sam_text_bytes"] == len(want) and len(z) < len(want) // 2
            check_pieces(walk_bgzf(z, eof=False), want)
        # a buffer below the worst case of the text is refused with that size; the fetch into one that holds it gives the members
        z, rep = m.map_text_se(se, sam_cap=len(plain_se) // 2)
        assert z is None and rep["reason"] == api.TEXT_SAM_CAP and rep["sam_bytes"] == api.bgzf_bound(len(plain_se)) - 28
        z, rep = m.fetch_text_sam(rep["sam_bytes"])
        check_pieces(walk_bgzf(z, eof=False), plain_se)
        # the deferred road, two chunks in flight
        res = m.map_text_se_stream(chunks)
        for (z, rep), want in zip(res, plain_chunks):
            assert rep["reason"] == api.TEXT_OK and rep["sam_bytes"] == len(z) and rep["sam_text_bytes"] == len(want)
            check_pieces(walk_bgzf(z, eof=False), want)
    finally:
        m.set_bgzf(False)
    assert m.map_text_se(se)[0] == plain_se


# ---- command line ----
def _run(args, **kw):
    r = subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def _no_pg(text):
    return [l for l in text.split(b"\n") if not l.startswith(b"@PG")]


def _records(text):
    return [l for l in text.split(b"\n") if l and not l.startswith(b"@")]


def _se_args(golden, out, fq=None):
    return ["-map", fq or os.path.join(GOLD, "se150.fq"), "-ufi", golden["ufi"], "-samout", out, "-quiet"]


@pytest.fixture(scope="module")
def plain_se(golden):
    out = os.path.join(golden["dir"], "plain_se.sam")
    _run(_se_args(golden, out))
    text = open(out, "rb").read()
    assert _records(text) == _records(gold("se150.sam"))
    return text


def test_cli_map_bgzf(golden, plain_se):
    out = os.path.join(golden["dir"], "se.sam.bgzf")
    r = _run(_se_args(golden, out)[:-1] + ["-bgzf"])
    blob = open(out, "rb").read()
    text = b"".join(m[0] for m in walk_bgzf(blob))
    assert _no_pg(text) == _no_pg(plain_se)
    pg = [l for l in text.split(b"\n") if l.startswith(b"@PG")]
    assert len(pg) == 1 and b"-bgzf" in pg[0]
    assert b"written as BGZF" in r.stderr and len(blob) < len(text) // 2


def test_cli_map2_bgzf(golden):
    base = ["-map2", os.path.join(GOLD, "pe150_1.fq"), "-reverse", os.path.join(GOLD, "pe150_2.fq"), "-ufi", golden["ufi"], "-quiet"]
    plain, out, tab = (os.path.join(golden["dir"], n) for n in ("plain_pe.sam", "pe.sam.bgzf", "pe.tab"))
    _run(base + ["-samout", plain])
    _run(base + ["-samout", out, "-tabbedout", tab, "-bgzf"])
    want = open(plain, "rb").read()
    assert _records(want) == _records(gold("pe150.sam"))
    text = b"".join(m[0] for m in walk_bgzf(open(out, "rb").read()))
    assert _no_pg(text) == _no_pg(want)
    assert open(tab, "rb").read() == gold("pe150.tab")  # -tabbedout stays plain text


def test_cli_shards_are_complete_files(golden, plain_se):
    out = os.path.join(golden["dir"], "sh.sam")
    _run(_se_args(golden, out) + ["-bgzf", "-samshards", "2", "-batch", "64"])
    blobs = [open(f"{out}.{s}", "rb").read() for s in range(2)]
    parts = [b"".join(m[0] for m in walk_bgzf(b)) for b in blobs]
    assert all(parts)
    assert _no_pg(b"".join(parts)) == _no_pg(plain_se)
    assert _no_pg(gzip.decompress(b"".join(blobs))) == _no_pg(plain_se)


def test_cli_stdout_pipe(golden, plain_se):
    r = subprocess.run(f"'{EXE}' -map '{os.path.join(GOLD, 'se150.fq')}' -ufi '{golden['ufi']}' -samout /dev/stdout -bgzf -quiet | cat",
                       shell=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert _no_pg(b"".join(m[0] for m in walk_bgzf(r.stdout))) == _no_pg(plain_se)


def test_cli_host_text_road(golden, plain_se):
    out = os.path.join(golden["dir"], "host.sam.bgzf")
    _run(_se_args(golden, out) + ["-bgzf"], env=dict(os.environ, URMAPX_HOST_TEXT="1"))
    assert _no_pg(b"".join(m[0] for m in walk_bgzf(open(out, "rb").read()))) == _no_pg(plain_se)


def test_cli_carriage_return_takes_the_host_fallback(golden):
    fq = os.path.join(golden["dir"], "cr.fq")
    lines = gold("se150.fq").split(b"\n")[:-1]
    lines[4 * 100 + 1] += b"\r"
    open(fq, "wb").write(b"\n".join(lines) + b"\n")
    plain, out = os.path.join(golden["dir"], "cr.sam"), os.path.join(golden["dir"], "cr.sam.bgzf")
    _run(_se_args(golden, plain, fq) + ["-batch", "64"])
    _run(_se_args(golden, out, fq) + ["-batch", "64", "-bgzf"])
    want = open(plain, "rb").read()
    assert _records(want) == _records(gold("se150.sam"))
    assert _no_pg(b"".join(m[0] for m in walk_bgzf(open(out, "rb").read()))) == _no_pg(want)


def test_cli_gz_input(golden, plain_se):
    fq = os.path.join(golden["dir"], "in.fq.gz")
    with gzip.open(fq, "wb") as f:
        f.write(gold("se150.fq"))
    out = os.path.join(golden["dir"], "gz.sam.bgzf")
    _run(_se_args(golden, out, fq) + ["-bgzf"])
    assert _no_pg(b"".join(m[0] for m in walk_bgzf(open(out, "rb").read()))) == _no_pg(plain_se)


def test_cli_gz_name_without_the_flag_is_plain_text(golden, plain_se):
    out = os.path.join(golden["dir"], "x.sam.gz")
    _run(_se_args(golden, out))
    assert _no_pg(open(out, "rb").read()) == _no_pg(plain_se)
