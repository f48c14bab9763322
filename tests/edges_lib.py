"""Seeded reads and pairs at the edges of sequences and of the sequence store (test infrastructure; numpy only).

Every other generator of the suite keeps its reads in the interior of a sequence.  AlignHSP's window arithmetic (alignhsp.cpp:98-150:
StartPosDB < StartPosQ, LeftTL >= LeftTHi, a '-' pad byte in a flank window, RightTHi >= TL clipped to TL - 1), ExtendPen's
SeedPosDB < SeedPosQ, the x-drop walk into the zero bytes behind the store and ScanPair's DBPos >= 1024 guard with its unclipped
windows (state2.cpp:99-133, scan.cpp:14-39) only act within a few dozen bases of a sequence's first or last base.  This module puts
reads exactly there, each tagged with family, sequence, side, strand, distance d from the edge and edit:

  flush     first or last base of the read = first or last base of a sequence, no edit (ungapped, POS = 1 / the last possible POS)
  sweep     d = 0 .. 33 and two far values; one substitution, a 1- to 3-base insertion or a 1- to 3-base deletion 4, 8, 14 or 22 bases
            from the read end that faces the edge; read lengths 100, 150, 151, 152, 250, 600, 1 024; every sequence, both sides
  overhang  1 .. 30 random bases past an edge
  chimera   the last m bases of sequence i followed by the first bases of sequence i + 1
  long      the sweep at fewer d, reads of 1 100 .. 1 400 bases (the general kernel's)
  pairs     fragments flush with either edge, a mate with a sweep edit at the edge (on the single-end store), and on the rescue store
            -- a 400-base repeat of 40 copies, the first copy 100 bases behind a sequence's start, the last 250 before its end --
            plus- and minus-anchored pairs whose repeat mate only State2::ScanPair can place, "easy" (ScanSlots finds it) and with
            every probe k-mer broken (the whole-read Viterbi), at the first, a middle and the last copy of every sequence, and
            minus anchors around store position 1 024

  gate      on a store of its own (gate_store): reads of an interior locus whose diverged copy lies at a sequence's edge -- the
            interior hit lowers the penalty cap under the copy's HSPs, which AlignHSP then turns away at its first test

`reference_defined` marks the cases in which nothing the reference does can touch a byte at or beyond SeqDataSize (what lies there is
the reference's allocator's business; this project defines it as 4 096 zero bytes).
"""
from __future__ import annotations

import hashlib

import numpy as np

from urmap_amd import synth

W = 24
SLOTS = 524309
PAD = 32  # '-' bytes between two sequences of a store (the index builder's)
ACGT = synth.ACGT
SE_LENGTHS = (3001, 2050, 1537, 2600, 1821)  # offsets 0, 3033, 5115, 6684, 9316, end 11137: six residues mod 32 and mod 64
SWEEP_D = tuple(range(34)) + (47, 90)
SWEEP_LENS = (100, 150, 151, 152, 250, 600, 1024)  # the instances of search_se_kernel
EDIT_AT = (4, 8, 14, 22)  # bases from the read end that faces the edge (the edit's outermost base is the e-th)
EDITS = (("sub", 1), ("ins", 1), ("ins", 2), ("ins", 3), ("del", 1), ("del", 2), ("del", 3))
OVERHANGS = (1, 2, 3, 5, 8, 12, 20, 30)
LONG_D = (0, 3, 12, 23, 24, 25, 26, 33, 90)
LONG_LENS = (1100, 1237, 1400)
REP_LEN, REP_COPIES, REP_HEAD, REP_TAIL = 400, 10, 100, 250
RESCUE_GAPS = (950, 953, 957, 946)  # unique bases between two copies, per sequence (other residues of the offsets again)


def _rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)]


def _sub(b):
    return ACGT[(int(np.nonzero(ACGT == b)[0][0]) + 1) % 4]


def se_store(seed=9001):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [(f"edge{i + 1}", _rnd(rng, L)) for i, L in enumerate(SE_LENGTHS)]


def rescue_store(seed=9002):
    rng = np.random.Generator(np.random.PCG64(seed))
    rep = _rnd(rng, REP_LEN)
    out = []
    for i, gap in enumerate(RESCUE_GAPS):
        parts = [_rnd(rng, REP_HEAD)]
        for j in range(REP_COPIES):
            parts += [rep.copy(), _rnd(rng, gap if j + 1 < REP_COPIES else REP_TAIL)]
        out.append((f"resc{i + 1}", np.concatenate(parts)))
    return out


def copy_start(si, j):
    return REP_HEAD + j * (REP_LEN + RESCUE_GAPS[si])


def layout(store):
    """(offset of every sequence in the store, SeqDataSize): sequences PAD bytes of '-' apart"""
    offs, o = [], 0
    for _, s in store:
        offs.append(o)
        o += len(s) + PAD
    return offs, o - PAD


def store_bytes(store):
    offs, tl = layout(store)
    sd = np.full(tl, ord("-"), np.uint8)
    for o, (_, s) in zip(offs, store):
        sd[o:o + len(s)] = s
    return sd


def digest(store, reads):
    """SHA-256 over the store's and the reads' bytes, labels included"""
    h = hashlib.sha256()
    for lab, s in store:
        h.update(lab.encode() + b"\0" + s.tobytes() + b"\0")
    for lab, s, _ in reads:
        h.update(lab.encode() + b"\0" + s.tobytes() + b"\0")
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------------------
# one read at an edge
# ---------------------------------------------------------------------------------------------------------------------------
def edge_read(rng, seq, side, d, L, edit, e, minus):
    """L bases whose alignment lies d bases from `side` ('L': the sequence's first base, 'R': its last) of seq, with `edit` =
    (kind, n) put e bases from the read end that faces the edge, reverse-complemented when minus.  The read is built in the
    sequence's orientation, facing end first for 'L' and last for 'R'; its reference span is L - n (insertion), L + n
    (deletion) or L bases."""
    kind, n = edit if edit else (None, 0)
    span = L - n if kind == "ins" else L + n if kind == "del" else L
    ref = seq[d:d + span] if side == "L" else seq[len(seq) - d - span:len(seq) - d]
    assert len(ref) == span, (len(seq), side, d, L, edit)
    r = ref if side == "L" else ref[::-1]  # facing end first
    if kind == "sub":
        r = r.copy()
        r[e - 1] = _sub(r[e - 1])
    elif kind == "ins":
        r = np.concatenate([r[:e - 1], _rnd(rng, n), r[e - 1:]])
    elif kind == "del":
        r = np.concatenate([r[:e - 1], r[e - 1 + n:]])
    if side == "R":
        r = r[::-1]
    r = np.ascontiguousarray(r, dtype=np.uint8)
    assert len(r) == L
    return synth.revcomp(r) if minus else r


def _q(n):
    return np.full(n, ord("I"), np.uint8)


def _add(reads, tags, s, **tag):
    tag["len"] = len(s)
    lab = "{family}_{seq}{side}{strand}_d{d}_{edit}_n{k}".format(k=len(reads), strand="-" if tag["minus"] else "+", **tag)
    reads.append((lab, s, _q(len(s))))
    tags.append(tag)


def se_cases(seed=9100, store=None):
    """the single-end list on the single-end store (all read lengths up to 1 024) -> (reads, tags)"""
    store = store or se_store()
    rng = np.random.Generator(np.random.PCG64(seed))
    reads, tags = [], []
    combos = [(ed, e) for ed in EDITS for e in EDIT_AT]  # 28
    k = 0
    for si, (_, seq) in enumerate(store):
        for side in "LR":
            for L in SWEEP_LENS:
                for minus in (False, True):
                    _add(reads, tags, edge_read(rng, seq, side, 0, L, None, 0, minus), family="flush", seq=si, side=side, minus=minus, d=0, edit="none")
                if L + 100 > len(seq):
                    continue
                for k, d in enumerate(SWEEP_D, 2 * si + (side == "R")):
                    # four of the 28 (edit, place) combinations per (edge, length, d), the next four at the next d and at the next
                    # length: over the seven lengths every d of every edge meets every combination; the strands alternate
                    for v in range(4):
                        ed, e = combos[(SWEEP_LENS.index(L) + k) % 7 + 7 * v]
                        minus = bool((k + v) & 1)
                        _add(reads, tags, edge_read(rng, seq, side, d, L, ed, e, minus), family="sweep", seq=si, side=side, minus=minus, d=d,
                             edit=f"{ed[0]}{ed[1]}at{e}")
            for oh in OVERHANGS:
                for L in (100, 150, 250):
                    minus = bool((oh + L) & 1)
                    inside = seq[:L - oh] if side == "L" else seq[len(seq) - (L - oh):]
                    r = np.concatenate([_rnd(rng, oh), inside] if side == "L" else [inside, _rnd(rng, oh)])
                    _add(reads, tags, synth.revcomp(r) if minus else r, family="overhang", seq=si, side=side, minus=minus, d=-oh, edit="none")
        if si + 1 < len(store):
            nxt = store[si + 1][1]
            for m in (1, 7, 24, 40, 75, 110, 126, 149):
                for minus in (False, True):
                    r = np.concatenate([seq[len(seq) - m:], nxt[:150 - m]])
                    _add(reads, tags, synth.revcomp(r) if minus else r, family="chimera", seq=si, side="R", minus=minus, d=-m, edit="none")
    return reads, tags


def se150_sweep(seed=9101, store=None):
    """every (edit, place) combination at every d, 150-base reads, both strands in turn: the list whose flips the golden fixtures
    are thinned from -> (reads, tags)"""
    store = store or se_store()
    rng = np.random.Generator(np.random.PCG64(seed))
    reads, tags = [], []
    k = 0
    for si, (_, seq) in enumerate(store):
        for side in "LR":
            for ed in EDITS:
                for e in EDIT_AT:
                    for d in SWEEP_D:
                        minus = bool(k & 1)
                        k += 1
                        _add(reads, tags, edge_read(rng, seq, side, d, 150, ed, e, minus), family="sweep", seq=si, side=side, minus=minus, d=d,
                             edit=f"{ed[0]}{ed[1]}at{e}")
    return reads, tags


def long_cases(seed=9102, store=None):
    """reads of 1 100 .. 1 400 bases: beyond the fast kernels -> (reads, tags)"""
    store = store or se_store()
    rng = np.random.Generator(np.random.PCG64(seed))
    reads, tags = [], []
    combos = [(ed, e) for ed in EDITS for e in EDIT_AT]
    k = 0
    for si, (_, seq) in enumerate(store):
        for side in "LR":
            for L in LONG_LENS:
                if L + 100 > len(seq):
                    continue
                _add(reads, tags, edge_read(rng, seq, side, 0, L, None, 0, bool(k & 1)), family="long_flush", seq=si, side=side, minus=bool(k & 1), d=0,
                     edit="none")
                for d in LONG_D:
                    ed, e = combos[(11 * k) % 28]
                    minus = bool(k & 1)
                    k += 1
                    _add(reads, tags, edge_read(rng, seq, side, d, L, ed, e, minus), family="long", seq=si, side=side, minus=minus, d=d,
                         edit=f"{ed[0]}{ed[1]}at{e}")
    return reads, tags


# ---------------------------------------------------------------------------------------------------------------------------
# pairs
# ---------------------------------------------------------------------------------------------------------------------------
def _add_pair(reads, tags, a, b, flip, **tag):
    """a: the fragment's forward-strand mate, b: its reverse-strand mate (already reverse-complemented); flip: b is mate 1"""
    tag["flip"] = flip
    lab = "{family}_{seq}{side}_d{d}_{edit}_n{k}".format(k=len(reads) // 2, **tag)
    m1, m2 = (b, a) if flip else (a, b)
    reads += [(lab + "/1", m1, _q(len(m1))), (lab + "/2", m2, _q(len(m2)))]
    tags.append(tag)


def pe_edge_cases(seed=9103, store=None, L=150, frag=300):
    """pairs on the single-end store: fragments flush with either edge of every sequence, and fragments whose mate at the edge has
    a sweep edit facing it -> (interleaved reads, one tag per pair)"""
    store = store or se_store()
    rng = np.random.Generator(np.random.PCG64(seed))
    reads, tags = [], []
    combos = [(ed, e) for ed in EDITS for e in EDIT_AT]
    k = 0
    for si, (_, seq) in enumerate(store):
        n = len(seq)
        for side in "LR":
            for idx, d in enumerate((0,) + SWEEP_D):
                for flip in (False, True):
                    swept = idx > 0  # the first two pairs of every edge: flush, no edit
                    ed, e = combos[(5 * k) % 28] if swept else (None, 0)
                    k += 1
                    if side == "L":  # the forward mate lies at the edge
                        a = edge_read(rng, seq, "L", d, L, ed, e, False)
                        b = synth.revcomp(seq[d + frag - L:d + frag])
                    else:  # the reverse mate lies at the edge
                        a = seq[n - d - frag:n - d - frag + L].copy()
                        b = edge_read(rng, seq, "R", d, L, ed, e, True)
                    _add_pair(reads, tags, a, b, flip, family="pe_sweep" if swept else "pe_flush", seq=si, side=side, d=d,
                              edit=f"{ed[0]}{ed[1]}at{e}" if swept else "none")
    return reads, tags


def _break_probes(s):
    """a substitution in each of ScanSlots' probe k-mers (query positions 0, 27, 54, 81), of either strand's coordinates"""
    s = s.copy()
    n = len(s)
    for p in (10, 35, 60, 90):
        for x in (p, n - 1 - p):
            s[x] = _sub(s[x])
    return s


def rescue_cases(seed=9104, store=None):
    """pairs on the rescue store -> (interleaved reads, one tag per pair).  anchor '+': the unique mate lies before the copy on the
    forward strand, ScanPair opens 1 024 bytes from its hit; '-': it lies behind the copy on the reverse strand, the window begins
    1 024 bytes before its hit (only where the hit is at store position >= 1 024) and is 1 024 + 2 QL long"""
    store = store or rescue_store()
    rng = np.random.Generator(np.random.PCG64(seed))
    reads, tags = [], []
    L = 150

    def pair(si, j, anchor, apos, mpos, broken, nsub, flip, family, QL=L):
        seq = store[si][1]
        n = len(seq)
        assert 0 <= apos and apos + QL <= n and 0 <= mpos and mpos + QL <= n, (si, j, anchor, apos, mpos)
        a = seq[apos:apos + QL].copy()
        m = seq[mpos:mpos + QL].copy()
        if broken:
            m = _break_probes(m)
        else:
            for t in range(nsub):
                m[100 + 7 * t] = _sub(m[100 + 7 * t])
        if anchor == "+":
            fwd, rev = a, synth.revcomp(m)
        else:
            fwd, rev = m, synth.revcomp(a)
        _add_pair(reads, tags, fwd, rev, flip, family=family, seq=si, side={0: "L", REP_COPIES - 1: "R"}.get(j, "M"), d=apos if anchor == "-" else n - apos,
                  edit=("broken" if broken else f"easy{nsub}") + anchor, anchor=anchor, copy=j)

    k = 0
    for si, (_, seq) in enumerate(store):
        n = len(seq)
        for j in (0, REP_COPIES // 2, REP_COPIES - 1):
            c = copy_start(si, j)
            for broken in (False, True):
                for v in range(4):
                    flip = bool(k & 1)
                    k += 1
                    # plus anchor: ends up to 50 bases inside the copy (at the first copy it begins at the sequence's first bases)
                    apos = max(0, c - 150 + 12 * v) if j else (0, 1, 7, 25)[v]
                    pair(si, j, "+", apos, c + 60 + 40 * v, broken, v, flip, "rescue")
                    # minus anchor: begins up to 50 bases inside the copy's end; at the last copy it ends at the sequence's last bases
                    apos = c + REP_LEN - 12 * v + 30 if j + 1 < REP_COPIES else n - 150 - (0, 1, 7, 25)[v]
                    pair(si, j, "-", apos, c + 40 + 40 * v, broken, v, not flip, "rescue")
        # 279-base mates (the longest the fast pair kernel takes) at the sequence's end: the minus anchor's window ends 2 x 279
        # bytes behind its hit, past the sequence (and, in the last sequence, past the store)
        c = copy_start(si, REP_COPIES - 1)
        for v, broken in enumerate((False, True)):
            pair(si, REP_COPIES - 1, "-", n - 279 - v, c + 30 + 50 * v, broken, 1, bool(v), "rescue279", QL=279)
            pair(si, REP_COPIES - 1, "+", c - 279 + 40, c + 90 + 20 * v, broken, 1, not v, "rescue279", QL=279)
    # minus anchors of the first sequence around store position 1 024: below it ScanPair does not scan (state2.cpp:111)
    c = copy_start(0, 0)
    for apos in list(range(874, 1020, 6)) + [1021, 1022, 1023, 1024, 1024, 1025, 1026, 1031]:
        for broken in (False, True):
            k += 1
            pair(0, 0, "-", apos, c + 100 + (apos % 5) * 20, broken, apos % 3, bool(k & 1), "rescue1024")
    return reads, tags


# ---------------------------------------------------------------------------------------------------------------------------
# the reference-defined subset
# ---------------------------------------------------------------------------------------------------------------------------
def slot_of(words, slots=SLOTS):
    """the index's slot of a W-mer given as its 2-bit word (first base most significant): the 64-bit murmur finalizer modulo the
    table size, as the oracle's uo_slots_vec computes it (test_edges_cpu.py compares the two)"""
    h = np.asarray(words, np.uint64).copy()
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xc4ceb9fe1a85ec53)
        h ^= h >> np.uint64(33)
    return h % np.uint64(slots)


class KmerTable:
    """the positions of a store that can seed -- the '-' pads break W-mers, W-mers with more than max_ix occurrences the index drops
    -- sorted by their slot in the index's table: a W-mer of a read seeds wherever a W-mer of the store shares its SLOT, equal
    or not (the table holds no words; 2 % of its slots are taken by an 11 kbp store, and a read asks for some hundreds)"""

    def __init__(self, store, max_ix=32, slots=SLOTS):
        self.sd = store_bytes(store)
        self.tl = len(self.sd)
        self.slots = slots
        code, ok = self._codes(self.sd)
        pos = np.nonzero(ok)[0]
        _, inv, cnt = np.unique(code[pos], return_inverse=True, return_counts=True)
        pos = pos[cnt[inv] <= max_ix]
        key = slot_of(code[pos], slots)
        order = np.argsort(key, kind="stable")
        self.codes = key[order]
        self.wordv = code[pos][order]
        self.pos = pos[order].astype(np.int64)

    @staticmethod
    def words(s):
        """(2-bit word of the W-mer at every position of s, first base most significant; False where it holds another letter)"""
        return KmerTable._codes(s)

    @staticmethod
    def _codes(s):
        lut = np.full(256, 4, np.uint64)
        for k, c in enumerate(b"ACGT"):
            lut[c] = k
        c = lut[s]
        n = max(0, len(s) - W + 1)
        v = np.zeros(n, np.uint64)
        ok = np.ones(n, bool)
        for j in range(W):
            cj = c[j:j + n]
            ok &= cj < 4
            v |= (cj & np.uint64(3)) << np.uint64(2 * (W - 1 - j))
        return v, ok

    def max_diagonal_end(self, read, reach_plus, reach_minus):
        """over every diagonal DBLo >= 0 at which a W-mer of `read` (plus: as it is, minus: reverse-complemented) shares its slot
        with a W-mer of the store: the largest DBLo + reach (0 if there is none).  Where the two W-mers differ nothing comes of the seed but
        ExtendPen's walk: reach = how far that walk gets (the read's length unless that would pass the store's end); where they are
        equal, the strand's reach"""
        best = 0
        for s, reach in ((read, reach_plus), (synth.revcomp(read), reach_minus)):
            v, ok = self._codes(s)
            q = np.nonzero(ok)[0]
            key = slot_of(v[q], self.slots)
            lo = np.searchsorted(self.codes, key, "left")
            hi = np.searchsorted(self.codes, key, "right")
            for t in range(int((hi - lo).max()) if len(q) else 0):
                m = lo + t < hi
                at = lo[m] + t
                dblo = self.pos[at] - q[m]
                same = self.wordv[at] == v[q[m]]
                end = dblo + np.where(same, reach, len(s))
                # a seed on a shared slot whose whole-read reach would pass the store's end: how far the walk really gets
                for k in np.nonzero((dblo >= 0) & ~same & (end > self.tl))[0]:
                    end[k] = dblo[k] + self._walk_end(s, int(q[m][k]), int(dblo[k]))
                end = end[dblo >= 0]
                if len(end):
                    best = max(best, int(end.max()))
        return best

    def _walk_end(self, s, qpos, dblo, mismatch=-3, xdrop=9):
        """one past the last read position ExtendPen's rightward x-drop walk compares, from a seed at qpos on diagonal dblo
        (extendpen.cpp:25-41 with method 6's constants; the penalty cap, which could only end the walk sooner, left out; bytes
        behind the store never match)"""
        score, best, p = W, 0, qpos + W
        while p < len(s):
            t = self.sd[dblo + p] if dblo + p < self.tl else 0
            p += 1
            if s[p - 1] == t:
                score += 1
                best = max(best, score)
            else:
                score += mismatch
                if best - score > xdrop:
                    break
        return p


def reference_defined(store, reads, pairs=False, max_ix=32):
    """bool per read (per pair with pairs=True): nothing the reference does for it can touch a byte at or beyond SeqDataSize.
    Single reads: DBLo + QL <= TL on every diagonal a W-mer of the read seeds (ExtendPen's walk; AlignHSP clips its right window
    itself).  Pairs: on every such diagonal of either mate also the window ScanPair could open from a hit there -- 1 024 bytes from
    a plus hit, 2 QL (of mate 1) behind a minus hit -- and ExtendScan's walk from a k-mer at the window's end (the other mate's
    length) end at or before TL, with a band's width to spare for a hit AlignHSP moved off its diagonal."""
    kt = KmerTable(store, max_ix)
    if not pairs:
        return np.array([kt.max_diagonal_end(s, len(s), len(s)) <= kt.tl for _, s, _ in reads])
    out = []
    for i in range(0, len(reads), 2):
        l1, l2 = len(reads[i][1]), len(reads[i + 1][1])
        e1 = kt.max_diagonal_end(reads[i][1], 1024 + l2 + 32, 2 * l1 + l2 + 32)
        e2 = kt.max_diagonal_end(reads[i + 1][1], 1024 + l1 + 32, 2 * l1 + l1 + 32)
        out.append(max(e1, e2) <= kt.tl)
    return np.array(out)


def select_flips(tags, outcomes, key=("seq", "side", "edit", "minus", "len")):
    """indices of the cases at which the outcome changes along d, and the case before each: the series are the cases that agree in
    `key`, in the order of d"""
    series = {}
    for i, t in enumerate(tags):
        series.setdefault(tuple(t.get(k) for k in key), []).append(i)
    pick = set()
    for idx in series.values():
        idx = sorted(idx, key=lambda i: tags[i]["d"])
        for a, b in zip(idx, idx[1:]):
            if outcomes[a] != outcomes[b]:
                pick.update((a, b))
    return sorted(pick)


# ---------------------------------------------------------------------------------------------------------------------------
# outcomes, from the oracle's results alone
# ---------------------------------------------------------------------------------------------------------------------------
UNMAPPED = 0xFFFFFFFF


def outcome(res):
    """per read: 'unmapped', 'ungapped' (a full-length hit of ExtendPen: no path) or 'gapped' (the hit came out of AlignHSP's or the
    rescue's DP: it carries a path)"""
    return np.where(res["dbpos"] == UNMAPPED, "unmapped", np.where(res["path_len"] > 0, "gapped", "ungapped"))


def outcome_table(tags, res, per_pair=False):
    """{family: {'n':, 'gapped':, 'ungapped':, 'unmapped':}} (reads; mates when per_pair)"""
    oc = outcome(res)
    out = {}
    for i, o in enumerate(oc):
        t = tags[i // 2] if per_pair else tags[i]
        a = out.setdefault(t["family"], {"n": 0, "gapped": 0, "ungapped": 0, "unmapped": 0})
        a["n"] += 1
        a[str(o)] += 1
    return out


def edit_kind(tag):
    return tag["edit"][:3]


# ---------------------------------------------------------------------------------------------------------------------------
# the thinned selections kept as golden fixtures (tests/golden/make_golden_edges.py), all inside the reference-defined subset
# ---------------------------------------------------------------------------------------------------------------------------
def golden_se(outcomes_of, store=None):
    """150-base reads: the flush reads of every edge, and of every second (edit, place) series of se150_sweep the cases at which
    the outcome flips along d with the case before each.  outcomes_of(reads) -> outcome per read (the oracle's, or read off the
    reference's SAM) -> (reads, tags)"""
    store = store or se_store()
    reads, tags = se150_sweep(store=store)
    oc = outcomes_of(reads)
    combos = [f"{ed[0]}{ed[1]}at{e}" for ed in EDITS for e in EDIT_AT]
    sel = [i for i in select_flips(tags, oc, key=("seq", "side", "edit"))
           if (combos.index(tags[i]["edit"]) + tags[i]["seq"] + (tags[i]["side"] == "R")) % 2 == 0]
    fr, ft = se_cases(store=store)
    flush = [i for i, t in enumerate(ft) if t["family"] == "flush" and t["len"] == 150]
    out_r = [fr[i] for i in flush] + [reads[i] for i in sel]
    out_t = [ft[i] for i in flush] + [tags[i] for i in sel]
    keep = reference_defined(store, out_r)
    return [r for r, k in zip(out_r, keep) if k], [t for t, k in zip(out_t, keep) if k]


def golden_pe(store=None):
    """pairs on the rescue store: every second rescue pair, the 279-base ones, the minus anchors from store position 1 010 on, and
    fragments at the edges of its sequences at d = 0, 12, 24, 25, 26, 90 -> (interleaved reads, tags)"""
    store = store or rescue_store()
    r, t = rescue_cases(store=store)
    pick = [i for i, x in enumerate(t) if x["family"] == "rescue279" or (x["family"] == "rescue" and i % 2 == 0)
            or (x["family"] == "rescue1024" and x["d"] >= 1010)]
    e, te = pe_edge_cases(seed=9105, store=store)
    pick_e = [i for i, x in enumerate(te) if x["d"] in (0, 12, 24, 25, 26, 90)]
    out_r = [y for i in pick for y in r[2 * i:2 * i + 2]] + [y for i in pick_e for y in e[2 * i:2 * i + 2]]
    out_t = [t[i] for i in pick] + [te[i] for i in pick_e]
    keep = reference_defined(store, out_r, pairs=True)
    return [y for i, k in enumerate(keep) if k for y in out_r[2 * i:2 * i + 2]], [x for x, k in zip(out_t, keep) if k]


def strip_mate_suffix(reads):
    """the labels as a FASTQ pair of files carries them: without /1 and /2"""
    return [(lab[:-2] if lab.endswith(("/1", "/2")) else lab, s, q) for lab, s, q in reads]


def sam_outcomes(records):
    """unmapped / ungapped / gapped per record of a single-end SAM (header lines skipped), as SAM shows it: a CIGAR with I or D is
    gapped (an alignment of AlignHSP's whose path is all M reads as ungapped here)"""
    out = []
    for l in records:
        if l.startswith(b"@"):
            continue
        f = l.split(b"\t")
        out.append("unmapped" if int(f[1]) & 4 else "gapped" if (b"I" in f[5] or b"D" in f[5]) else "ungapped")
    return np.array(out)


# ---------------------------------------------------------------------------------------------------------------------------
# a second, worse locus at an edge: the HSPs a lowered penalty cap leaves unaligned
# ---------------------------------------------------------------------------------------------------------------------------
GATE_SEQ_LEN, GATE_AT, GATE_COPY = 2400, 1000, 160
GATE_SUBS = (10, 36, 42, 48, 54, 100, 106, 112, 138, 144)  # five in either half, 25 bases without one in each (two shared 24-mers)
GATE_D = (0, 10, 26)


def gate_store(seed=9005):
    """six sequences of random ACGT; each holds, GATE_D bases from its first (gate1..3) or last (gate4..6) base, a copy of its own
    interior bases [1000, 1160) with the substitutions GATE_SUBS: two 24-mers of either half occur at both places"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(2 * len(GATE_D)):
        s = _rnd(rng, GATE_SEQ_LEN)
        e = s[GATE_AT:GATE_AT + GATE_COPY].copy()
        for p in GATE_SUBS:
            e[p] = _sub(e[p])
        lo = gate_copy_start(i)
        s[lo:lo + GATE_COPY] = e
        out.append((f"gate{i + 1}", s))
    return out


def gate_copy_start(si):
    d = GATE_D[si % len(GATE_D)]
    return d if si < len(GATE_D) else GATE_SEQ_LEN - GATE_COPY - d


def gate_cases(seed=9106, store=None):
    """150-base reads from the interior locus with one 1-base deletion or insertion near the middle.  The 24-mers that span a
    substitution of the copy are unique: phases 1-2 find the interior locus' two HSPs first (either side of the indel, under 60 % of
    the read each: no phase 3).  The shared 24-mers bring the copy's two HSPs in phase 4, five substitutions (penalty 20) each.
    Phase 6 aligns the first two into a hit of penalty 5 or 6, which lowers the cap to 11 or 12 -- AlignHSP returns at its first
    test for the copy's HSPs (the device gates their jobs before the DP), which at d = 0 and 10 would fail the window tests
    otherwise -> (reads, tags)"""
    store = store or gate_store()
    rng = np.random.Generator(np.random.PCG64(seed))
    reads, tags = [], []
    for si, (_, seq) in enumerate(store):
        for k, at in enumerate((66, 70, 74, 78, 82, 86)):
            for kind in ("del", "ins"):
                minus = bool((k + (kind == "ins")) & 1)
                lo = GATE_AT + 2 + k % 3
                ref = seq[lo:lo + (151 if kind == "del" else 149)]
                r = np.concatenate([ref[:at], ref[at + 1:]] if kind == "del" else [ref[:at], _rnd(rng, 1), ref[at:]])
                r = np.ascontiguousarray(r, dtype=np.uint8)
                _add(reads, tags, synth.revcomp(r) if minus else r, family="gate", seq=si, side="L" if si < len(GATE_D) else "R", minus=minus,
                     d=GATE_D[si % len(GATE_D)], edit=f"{kind}1at{at}")
    return reads, tags
