"""BGZF output, host side: a walker that checks a BGZF file member by member, and urmapx_bgzf_compress_host through it.
The walker is what tests/test_gpu_bgzf.py checks the device compressor and `urmap ... -bgzf` with."""
import gzip
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from urmap_amd import api  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
PIECE = 65280
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SAN = os.path.join(ROOT, "urmap_amd", "csrc", "build_san", "urmap_san_asan")


def walk_bgzf(blob, eof=True):
    """Checks every member of a BGZF byte string -> [(text bytes, deflate block type of the member's first block, member size)].
    eof: the last member must be htslib's 28-byte end-of-file marker (not part of the returned list)."""
    assert len(EOF_MEMBER) == 28
    members, at = [], 0
    while at < len(blob):
        head = blob[at:at + 18]
        assert len(head) == 18, "truncated member header"
        assert head[:4] == b"\x1f\x8b\x08\x04", f"magic / CM / FLG=FEXTRA at {at}: {head[:4].hex()}"
        xlen, = struct.unpack("<H", head[10:12])
        assert xlen == 6 and head[12:14] == b"BC" and head[14:16] == b"\x02\x00", f"BC subfield at {at}"
        bsize = struct.unpack("<H", head[16:18])[0] + 1
        assert at + bsize <= len(blob), f"BSIZE at {at} runs past the end"
        body = blob[at + 18:at + bsize - 8]
        crc, isize = struct.unpack("<II", blob[at + bsize - 8:at + bsize])
        assert isize <= PIECE, f"ISIZE {isize} at {at}"
        d = zlib.decompressobj(-15)
        text = d.decompress(body) + d.flush()
        assert d.eof and d.unused_data == b"", f"deflate stream of the member at {at} does not end with its body"
        assert len(text) == isize, (len(text), isize)
        assert zlib.crc32(text) == crc, f"CRC-32 of the member at {at}"
        members.append((text, (body[0] >> 1) & 3, bsize, blob[at:at + bsize]))
        at += bsize
    assert at == len(blob)  # BSIZE chains from member to member up to exactly the end
    if eof:
        assert members and members[-1][3] == EOF_MEMBER, "no end-of-file member"
        members.pop()
    assert all(len(m[0]) > 0 for m in members), "an empty member that is not the end-of-file marker"
    whole = b"".join(m[0] for m in members)
    if blob:
        assert gzip.decompress(blob) == whole
    return [(m[0], m[1], m[2]) for m in members]


def check_pieces(members, data):
    """the members hold `data` cut every 65 280 bytes, and none is larger than its text + 31"""
    assert b"".join(m[0] for m in members) == data
    want = [min(PIECE, len(data) - o) for o in range(0, len(data), PIECE)]
    assert [len(m[0]) for m in members] == want
    for text, _, size in members:
        assert size <= len(text) + 31


def seeded_bytes(n, seed=7):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def lib():
    return api.lib()  # (a library that does not load is a failure)


@pytest.fixture(scope="module")
def san():
    """the sanitizer build of the host side, made current (as tests/test_sanitizers_cpu.py does)"""
    if not shutil.which("g++"):
        pytest.skip("no g++ for the sanitizer builds")
    r = subprocess.run(["make", "-s", "-j3", "-C", os.path.join(ROOT, "urmap_amd", "csrc"), "san"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.exists(SAN)
    return SAN


def test_walker_accepts_what_it_should_and_nothing_else():
    def member(text):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(text) + c.flush()
        return (b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25) + body
                + struct.pack("<II", zlib.crc32(text), len(text)))
    good = member(b"hello\n" * 100) + member(b"world") + EOF_MEMBER
    assert [m[0] for m in walk_bgzf(good)] == [b"hello\n" * 100, b"world"]
    bad_crc = bytearray(good); bad_crc[len(member(b"hello\n" * 100)) - 8] ^= 1
    for blob in (good[:-28], bytes(bad_crc), good + b"\0", gzip.compress(b"hello")):
        with pytest.raises(AssertionError):
            walk_bgzf(bytes(blob))


def test_bound(lib):
    assert api.bgzf_bound(0) == 28
    assert api.bgzf_bound(1) == 1 + 31 + 28
    assert api.bgzf_bound(PIECE) == PIECE + 31 + 28
    assert api.bgzf_bound(PIECE + 1) == PIECE + 1 + 62 + 28


def test_host_golden_sam(lib):
    data = open(os.path.join(GOLD, "se150.sam"), "rb").read()
    z = api.bgzf_compress_host(data)
    check_pieces(walk_bgzf(z), data)
    assert len(z) < len(data) // 2
    # without the end-of-file member: the same members
    assert api.bgzf_compress_host(data, eof=False) + EOF_MEMBER == z


def test_host_empty(lib):
    assert api.bgzf_compress_host(b"") == EOF_MEMBER
    assert api.bgzf_compress_host(b"", eof=False) == b""


@pytest.mark.parametrize("n", [1, PIECE - 1, PIECE, PIECE + 1])
def test_host_piece_cuts(lib, n):
    data = (open(os.path.join(GOLD, "se150.sam"), "rb").read() * 2)[:n]
    assert len(data) == n
    check_pieces(walk_bgzf(api.bgzf_compress_host(data)), data)


def test_host_random_is_stored(lib):
    data = seeded_bytes(200000)
    z = api.bgzf_compress_host(data)
    members = walk_bgzf(z)
    check_pieces(members, data)
    assert all(btype == 0 for _, btype, _ in members)
    assert len(z) <= len(data) + 31 * len(members) + 28


def test_host_cap_below_bound(lib):
    data = b"ACGT" * 1000
    with pytest.raises(api.UrmapxError) as e:
        api.bgzf_compress_host(data, cap=api.bgzf_bound(len(data)) - 1)
    assert e.value.code == -5


@pytest.mark.parametrize("extra", [[], ["-shards", "2"], ["-batch", "64", "-streams", "3"]])
def test_pipeline_bgzf_under_asan(tmp_path, san, extra):
    """urmapx_map_files with bgzf set, host side under ASan + UBSan with the device stand-in: header, lane chunks, end-of-file member,
    shards -- the bytes inflate to the plain run's."""
    fq = os.path.join(GOLD, "se150.fq")
    env = dict(os.environ, URX_STUB_MAP="1", ASAN_OPTIONS="exitcode=99:detect_leaks=0", UBSAN_OPTIONS="exitcode=99:halt_on_error=1")
    plain, z = str(tmp_path / "p.sam"), str(tmp_path / "z.sam")
    for out, flag in ((plain, []), (z, ["-bgzf"])):
        r = subprocess.run([SAN, "map", fq, "-o", out] + extra + flag, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    shards = 2 if "-shards" in extra else 0
    names = [f".{s}" for s in range(shards)] if shards else [""]
    text = b"".join(open(plain + s, "rb").read() for s in names)
    got = b""
    for s in names:
        blob = open(z + s, "rb").read()
        got += b"".join(m[0] for m in walk_bgzf(blob))
    assert got == text and len(text) > 100000
    if shards:
        assert gzip.decompress(b"".join(open(z + s, "rb").read() for s in names)) == text
