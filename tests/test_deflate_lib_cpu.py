"""tests/deflate_lib.py against things that are not the device compressor: its reader on zlib's own streams, its package-merge against
exhaustive search, its Huffman cost and depth against each other and against Fibonacci counts, whose tree is a known chain."""
import itertools
import zlib

import numpy as np
import pytest

import deflate_lib as dl
from test_bgzf_cpu import PIECE, seeded_bytes
from test_gpu_bgzf import EDGE, edge_input, gold

SAMS = ("se150.sam", "se250.sam", "pe150.sam", "pe100_noisy.sam")


def pieces_of(data):
    return [data[o:o + PIECE] for o in range(0, len(data), PIECE)]


def texts():
    out = [(f"{n}[{i}]", p) for n in SAMS for i, p in enumerate(pieces_of(gold(n)))]
    out += [(f"{n}[{i}]", p) for n in EDGE for i, p in enumerate(pieces_of(edge_input(n)))]
    return out


def deflate(text, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(text) + c.flush()


def read_and_check(body, text, want_types):
    blocks = dl.read_stream(body)
    assert {b.btype for b in blocks} <= want_types, [b.btype for b in blocks]
    tokens = [t for b in blocks for t in b.tokens]
    assert dl.replay(tokens) == text
    assert 8 * (len(body) - 1) < blocks[-1].end_bit <= 8 * len(body)
    for b in blocks:
        for t in b.tokens:
            assert isinstance(t, int) or (3 <= t[0] <= 258 and 1 <= t[1] <= 32768)
        if b.btype == 2:
            # what the header says about itself: the code-length code decodes its own sequence, zlib's codes are complete
            assert dl.kraft_units(b.cl_lengths, 7) <= 1 << 7 and dl.kraft_units(b.ll_lengths, 15) == 1 << 15
            assert all(b.cl_lengths[s] for s in b.cl_seq)
    return blocks


@pytest.mark.parametrize("level", [1, 6, 9])
def test_reader_on_zlib_streams(level):
    for name, text in texts():
        blocks = read_and_check(deflate(text, level), text, {0, 1, 2})
        if name.split("[")[0] in SAMS:  # (so the dynamic header's reader has run: 12 pieces)
            assert any(b.btype == 2 for b in blocks), name


def test_reader_on_fixed_code_streams():
    for name, text in texts():
        # (Z_FIXED rules out dynamic codes only: what does not shrink is still stored)
        read_and_check(deflate(text, 6, zlib.Z_FIXED), text, {1} if name.split("[")[0] in SAMS else {0, 1})


def test_reader_on_stored_streams():
    for n, seed in ((600, 2), (PIECE, 3), (100000, 4)):  # (zlib cuts stored blocks at 65 535 bytes)
        text = seeded_bytes(n, seed)
        blocks = read_and_check(deflate(text, 6), text, {0})
        assert sum(len(b.tokens) for b in blocks) == n
    text = seeded_bytes(3000, 5)
    read_and_check(deflate(text, 0), text, {0})


def test_reader_refuses_damage():
    text = gold("se150.sam")[:5000]
    body = deflate(text, 6)
    with pytest.raises(dl.DeflateError):
        dl.read_stream(body[:len(body) // 2])
    with pytest.raises(dl.DeflateError):
        dl.replay([65, (3, 2)])
    with pytest.raises(dl.DeflateError):
        dl._decoder([1, 1, 1])


def test_histograms_use_the_rfc_symbol_tables():
    assert [dl.LEN_SYMBOL[l] for l in (3, 10, 11, 12, 13, 18, 19, 130, 131, 226, 227, 257, 258)] == \
        [257, 264, 265, 265, 266, 268, 269, 280, 281, 283, 284, 284, 285]
    assert [dl.dist_symbol(d) for d in (1, 4, 5, 6, 7, 8, 9, 12, 13, 24576, 24577, 32768)] == [0, 3, 4, 4, 5, 5, 6, 6, 7, 28, 29, 29]
    ll, dd = dl.histograms([65, 65, (258, 1), (3, 32768), 66])
    assert (ll[65], ll[66], ll[256], ll[257], ll[285], sum(ll)) == (2, 1, 1, 1, 1, 6) and (dd[0], dd[29], sum(dd)) == (1, 1, 2)
    # against zlib: every symbol the tokens use has a code in the block that holds them
    text = gold("se150.sam")[:PIECE]
    for b in dl.read_stream(deflate(text, 6)):
        ll, dd = dl.histograms(b.tokens)
        assert all((c > 0) <= (l > 0) for c, l in zip(ll, b.ll_lengths)) and all((c > 0) <= (l > 0) for c, l in zip(dd, b.d_lengths))


def complete_codes(n, L):
    """every assignment of lengths 1..L to n symbols that is a complete prefix code, as rows"""
    rows = [t for t in itertools.product(range(1, L + 1), repeat=n) if sum(1 << (L - l) for l in t) == 1 << L]
    return np.array(rows, dtype=np.int64).reshape(len(rows), n)


@pytest.mark.parametrize("L", [2, 3, 4])
def test_package_merge_against_exhaustive_search(L):
    """every alphabet of 2..6 symbols with counts in 1..8 (both costs are symmetric in the symbols, so each multiset of counts once, in
    rising order, while the search still runs over every ordered assignment of lengths)"""
    checked = 0
    for n in range(2, 7):
        alphabets = np.array(list(itertools.combinations_with_replacement(range(1, 9), n)), dtype=np.int64)
        if n > 1 << L:
            with pytest.raises(ValueError):
                dl.package_merge_cost(list(alphabets[0]), L)
            continue
        codes = complete_codes(n, L)
        assert len(codes)
        best = (alphabets @ codes.T).min(axis=1)
        for counts, want in zip(alphabets, best):
            assert dl.package_merge_cost(list(counts), L) == want, (counts, L)
        checked += len(alphabets)
    assert checked >= 36 + 120 + 330 + (792 + 1716) * (L > 2)
    assert dl.package_merge_cost([0, 5, 0, 3, 8, 0, 1], L) == dl.package_merge_cost([1, 3, 5, 8], L)


def seeded_histograms(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        k = int(rng.integers(2, 287))
        kind = rng.integers(0, 3)
        if kind == 0:
            c = rng.integers(1, 1000, k)
        elif kind == 1:
            c = np.floor(rng.uniform(1.1, 2.2) ** np.arange(min(k, 30))).astype(np.int64)
        else:
            c = rng.geometric(0.02, k)
        yield [int(x) for x in rng.permutation(c)]


def test_package_merge_without_a_binding_limit_is_huffman():
    n = 0
    for counts in seeded_histograms(300, 5):
        h = dl.huffman_cost(counts)
        assert dl.package_merge_cost(counts, 32) == h
        d = dl.huffman_depth(counts)
        assert dl.package_merge_cost(counts, d) == h
        if d > (len(counts) - 1).bit_length():
            assert dl.package_merge_cost(counts, d - 1) > h
        for L in range(max(1, (len(counts) - 1).bit_length()), d):
            assert dl.package_merge_cost(counts, L) >= dl.package_merge_cost(counts, L + 1) > 0
        n += 1
    assert n == 300


@pytest.mark.parametrize("n", [2, 3, 8, 11, 16, 17, 23, 30])
def test_fibonacci_counts_make_a_chain(n):
    fib = [1, 1]
    while len(fib) < n:
        fib.append(fib[-1] + fib[-2])
    assert dl.huffman_depth(fib) == n - 1
    # the chain's cost: the two rarest at depth n - 1, then one symbol per level
    assert dl.huffman_cost(fib) == sum(c * d for c, d in zip(fib, [n - 1] + list(range(n - 1, 0, -1))))
    assert dl.kraft_units([n - 1] + list(range(n - 1, 0, -1)), n - 1) == 1 << (n - 1)


def test_small_cases():
    assert dl.huffman_cost([]) == 0 and dl.huffman_cost([0, 7]) == 7 and dl.huffman_depth([0, 7]) == 1 and dl.huffman_depth([0]) == 0
    assert dl.huffman_cost([1, 1]) == 2 and dl.huffman_depth([3, 0, 9]) == 1
    assert dl.huffman_cost([1] * 286) == 286 * 9 - (512 - 286)  # 226 codes of 8 bits, 60 of 9
    assert dl.huffman_depth([1] * 286) == 9
    assert dl.kraft_units([1, 2, 0, 2], 15) == 1 << 15
