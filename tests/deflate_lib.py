"""A plain DEFLATE reader (RFC 1951) and reference prefix codes, in Python, for judging the device compressor (bgzf_gpu.hip) from
what it wrote: the code lengths and the tokens of a block, the histograms they imply, and what the best code for a histogram
costs -- unlimited (Huffman, by a heap) and limited to L bits (package-merge).  Nothing here is taken from the kernel;
tests/test_deflate_lib_cpu.py checks it against zlib's output and against exhaustive search."""
import heapq
from types import SimpleNamespace

# RFC 1951 3.2.5: length symbols 257..285 and distance symbols 0..29, (base, extra bits)
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
LEN_BASE = []
_b = 3
for _e in LEN_EXTRA[:-1]:
    LEN_BASE.append(_b)
    _b += 1 << _e
LEN_BASE.append(258)
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in range(2)]
DIST_BASE = []
_b = 1
for _e in DIST_EXTRA:
    DIST_BASE.append(_b)
    _b += 1 << _e
assert len(LEN_BASE) == 29 and LEN_BASE[27] == 227 and len(DIST_BASE) == 30 and DIST_BASE[29] == 24577 and _b == 32769
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
NLL, ND, NCL = 286, 30, 19

LEN_SYMBOL = [None] * 259  # length -> symbol (258 is symbol 285, not 284 with all extra bits set)
for _s in range(28):
    for _l in range(LEN_BASE[_s], LEN_BASE[_s] + (1 << LEN_EXTRA[_s])):
        if _l < 258:
            LEN_SYMBOL[_l] = 257 + _s
LEN_SYMBOL[258] = 285


def dist_symbol(dist):
    s = 29
    while DIST_BASE[s] > dist:
        s -= 1
    return s


class DeflateError(ValueError):
    pass


class _Bits:
    def __init__(self, data, pos=0):
        self.data, self.pos, self.end = data, pos, 8 * len(data)

    def peek(self, n):  # up to 25 bits; bits behind the end read as 0
        i = self.pos >> 3
        return (int.from_bytes(self.data[i:i + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def take(self, n):
        if self.pos + n > self.end:
            raise DeflateError("the body ends inside a field")
        v = self.peek(n)
        self.pos += n
        return v


def _decoder(lengths):
    """code lengths -> (table over the next `width` bits of an LSB-first stream: (symbol, length) or None, width).  Canonical codes,
    RFC 1951 3.2.2.  An oversubscribed set of lengths is an error, an incomplete one leaves entries empty (as zlib allows)."""
    width = max(lengths) if lengths else 0
    if width == 0:
        return [None], 0
    count = [0] * (width + 1)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * (width + 1)
    for b in range(1, width + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    if sum(count[b] << (width - b) for b in range(1, width + 1)) > 1 << width:
        raise DeflateError("oversubscribed code")
    table = [None] * (1 << width)
    for s, l in enumerate(lengths):
        if not l:
            continue
        c = nxt[l]
        nxt[l] += 1
        r = int(format(c, f"0{l}b")[::-1], 2)
        for k in range(r, 1 << width, 1 << l):
            table[k] = (s, l)
    return table, width


def _symbol(bits, dec):
    table, width = dec
    e = table[bits.peek(width)] if width else None
    if e is None:
        raise DeflateError("a bit pattern that is no code")
    if bits.pos + e[1] > bits.end:
        raise DeflateError("the body ends inside a code")
    bits.pos += e[1]
    return e[0]


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30  # (symbols 30 and 31 of the fixed code never occur)


def read_block(body, bit=0):
    """One deflate block of `body` that starts at bit `bit` -> a namespace:
    bfinal, btype (0 stored, 1 fixed, 2 dynamic), tokens (a literal byte as an int, a match as (length, distance)), end_bit (the bit behind
    the end-of-block symbol; behind the last byte of a stored block), ll_lengths / d_lengths (the codes in force; None when stored), and
    for a dynamic block hlit, hdist, hclen (as counts: 257.., 1.., 4..), cl_lengths (19, by symbol) and cl_seq (the header's code-length
    symbols in order, 0..18, extra bits dropped)."""
    bits = _Bits(body, bit)
    B = SimpleNamespace(bfinal=bits.take(1), btype=bits.take(2), tokens=[], ll_lengths=None, d_lengths=None, hlit=None, hdist=None,
                        hclen=None, cl_lengths=None, cl_seq=None)
    if B.btype == 3:
        raise DeflateError("block type 3")
    if B.btype == 0:
        bits.pos = (bits.pos + 7) & ~7
        n, nn = bits.take(16), bits.take(16)
        if n ^ nn != 0xffff:
            raise DeflateError("LEN / NLEN")
        at = bits.pos >> 3
        if at + n > len(body):
            raise DeflateError("the body ends inside a stored block")
        B.tokens = list(body[at:at + n])
        B.end_bit = 8 * (at + n)
        return B
    if B.btype == 1:
        B.ll_lengths, B.d_lengths = list(FIXED_LL), list(FIXED_D)
    else:
        B.hlit, B.hdist, B.hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
        if B.hlit > NLL or B.hdist > ND:
            raise DeflateError("HLIT / HDIST")
        B.cl_lengths = [0] * NCL
        for i in range(B.hclen):
            B.cl_lengths[CL_ORDER[i]] = bits.take(3)
        dec = _decoder(B.cl_lengths)
        lens, B.cl_seq = [], []
        while len(lens) < B.hlit + B.hdist:
            s = _symbol(bits, dec)
            B.cl_seq.append(s)
            if s < 16:
                lens.append(s)
            elif s == 16:
                if not lens:
                    raise DeflateError("repeat with nothing before it")
                lens += [lens[-1]] * (3 + bits.take(2))
            elif s == 17:
                lens += [0] * (3 + bits.take(3))
            else:
                lens += [0] * (11 + bits.take(7))
        if len(lens) != B.hlit + B.hdist:
            raise DeflateError("a run crosses the end of the code lengths")
        B.ll_lengths, B.d_lengths = lens[:B.hlit] + [0] * (NLL - B.hlit), lens[B.hlit:] + [0] * (ND - B.hdist)
        if not B.ll_lengths[256]:
            raise DeflateError("no code for the end of the block")
    ll, dd = _decoder(B.ll_lengths), _decoder(B.d_lengths)
    tokens = B.tokens
    while True:
        s = _symbol(bits, ll)
        if s < 256:
            tokens.append(s)
        elif s == 256:
            break
        elif s > 285:
            raise DeflateError("length symbol 286 / 287")
        else:
            length = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
            d = _symbol(bits, dd)
            tokens.append((length, DIST_BASE[d] + bits.take(DIST_EXTRA[d])))
    B.end_bit = bits.pos
    return B


def read_stream(body):
    """every block of a raw deflate stream, up to and with the final one -> list of read_block's results"""
    blocks, bit = [], 0
    while True:
        blocks.append(read_block(body, bit))
        bit = blocks[-1].end_bit
        if blocks[-1].bfinal:
            return blocks


def replay(tokens):
    """the text a token list stands for (a distance that reaches before the text's start is an error)"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        length, dist = t
        if dist > len(out):
            raise DeflateError(f"distance {dist} at position {len(out)}")
        if dist >= length:
            out += out[len(out) - dist:len(out) - dist + length]
        else:
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out)


def histograms(tokens):
    """-> (286 literal/length counts, the end-of-block symbol counted once; 30 distance counts)"""
    ll, dd = [0] * NLL, [0] * ND
    for t in tokens:
        if isinstance(t, int):
            ll[t] += 1
        else:
            ll[LEN_SYMBOL[t[0]]] += 1
            dd[dist_symbol(t[1])] += 1
    ll[256] += 1
    return ll, dd


def cost(counts, lengths):
    return sum(c * l for c, l in zip(counts, lengths))


def huffman_cost(counts):
    """sum of count * length of an optimal prefix code without a length limit; a lone symbol costs one bit each time"""
    h = [c for c in counts if c]
    if len(h) < 2:
        return sum(h)
    heapq.heapify(h)
    total = 0
    while len(h) > 1:
        a = heapq.heappop(h) + heapq.heappop(h)
        total += a
        heapq.heappush(h, a)
    return total


def package_merge_cost(counts, L):
    """sum of count * length of an optimal prefix code whose lengths are at most L (Larmore and Hirschberg's package-merge, in its
    plain form: L lists of the sorted counts, each list's pairs carried into the next; the 2m - 2 cheapest of the last list)"""
    items = sorted(c for c in counts if c)
    m = len(items)
    if m > 1 << L:
        raise ValueError(f"{m} symbols do not fit a code of {L} bits")
    if m < 2:
        return sum(items)
    merged = items
    for _ in range(L - 1):
        packages = [merged[i] + merged[i + 1] for i in range(0, len(merged) - 1, 2)]
        merged = sorted(items + packages)
    return sum(merged[:2 * m - 2])


def huffman_depth(counts):
    """the least maximal length over all optimal unlimited codes: the smallest L at which the limit costs nothing"""
    m = sum(1 for c in counts if c)
    if m < 2:
        return m
    best = huffman_cost(counts)
    L = (m - 1).bit_length()
    while package_merge_cost(counts, L) != best:
        L += 1
    return L


def kraft_units(lengths, L):
    """sum of 2^(L - length) over the symbols in use: 2^L for a complete code"""
    assert all(l <= L for l in lengths)
    return sum(1 << (L - l) for l in lengths if l)
