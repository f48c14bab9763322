"""Seeded pairs placed at the decisions that depend on where two mates lie relative to each other (test infrastructure; numpy only).

Every other generator of the suite draws FR pairs of equal mates from one sequence, inserts around 300.  The reference decides at
five places by the mates' geometry -- the seed loop's and the 90 % shortcut's |DBStart_f - DBStart_r| + (Lf + Lr) / 2 <= 1000
(search2m4.cpp), FindPairs' same limit with opposite strands (state2.cpp:20-85), ScanPair's windows (state2.cpp:87-137) and SetSAM2's
TLEN / 0x2 / RNEXT / PNEXT rules (output2.cpp:61-128) -- and this module puts pairs one base either side of each, one tag dict per
pair (family, d, Lf, Lr, orient, flip, nsub, and each mate's sequence, coordinate, store position and strand):

  distance     FR pairs of lengths (left, right) = (150,150), (100,151), (151,100), (279,279), (64,250): the start-to-start store
               distance d through every value at which d + (Lf + Lr) / 2 = 996 .. 1004, at which TLEN = d + right length =
               996 .. 1004, and 1023 - Lr, 1024 - Lr, 1025 - Lr, 1023, 1024, 1025, 1500 (the scan windows' ends); each with 0, 2 and 5
               evenly spaced substitutions per mate.  One more series (`near`), 64/250 at d = 841 .. 846 at four anchors: two
               substitutions side by side in the short mate (score 56 of 64, under the 90 % shortcut's 57) beside an exact long
               mate -- only the seed loop gives such a pair MAPQ 40
  orientation  FR, RF, FF, RR at d = 0, 1, 60, 300, 849, 850, 851, mates 150/150 and 250/100 (the short one inside the long one
               while d <= 150), 0 and 5 substitutions; dovetails: the minus mate begins 1, 10, 149 bases left of the plus mate
  neighbours   mates on adjacent sequences of 380 .. 420 bases (left mate 0, 1, 20, 150 bases before its sequence's end, right
               mate 0, 1, 10 bases behind the next one's start; and the left mate near its sequence's start, the right one deep in
               the next), a short sequence followed by a long one with the right mate at 600 and at 1 200, and a same-sequence
               pair with a mate at coordinate 0
  choice       one sequence with seven groups of copies of a 150-base locus (exact, 2 and 4 substitutions; a locus per group), an
               anchor locus on either side of each group: one copy within the limit and a better one beyond, two within with
               different scores in either order, two exact ones, three in two orders; the mate at the copies is the locus with 3
               substitutions of its own
  lonely       the partner is random ACGT: plus anchors, minus anchors above store position 1 024 and below it

670 pairs in all (cases()).  Mate order (flip: the minus-strand or right-hand mate is mate 1) alternates in every family.  The store
ends in a ballast sequence that holds no case; its last bases are drawn (BALLAST_TAIL_SEED) so that no W-mer of any read shares an
index slot with a W-mer close enough to the store's end for ExtendPen's walk to pass it: edges_lib.reference_defined holds for
every pair.
"""
from __future__ import annotations

import numpy as np

import edges_lib as el
from urmap_amd import synth

W, SLOTS, PAD = el.W, el.SLOTS, el.PAD
MAX_TL = 1000
SEQS = (("geoA", 6000), ("geoB", 6100), ("nb1", 400), ("nb2", 390), ("nb3", 410), ("nb4", 400), ("nbL", 3000), ("choice", 18500),
        ("ballast", 2600))
SEQ_INDEX = {n: i for i, (n, _) in enumerate(SEQS)}
LENGTH_PAIRS = ((150, 150), (100, 151), (151, 100), (279, 279), (64, 250))  # (left mate, right mate)
LOADS = (0, 2, 5)
NEAR_SUBS = (30, 33)  # two substitutions that leave the 64-base mate its seeds
# anchors of the `near` series in geoB.  The seed loop compares the positions of the seeds' k-mers, not of the reads' first bases: a
# second seed of either mate (the read's next k-mer on another diagonal, after a k-mer that shares its slot with some other place)
# lies elsewhere in its read and can bring a pair under the limit whose first bases are beyond it.  At these anchors, found with
# the oracle, none does: the first seeds decide, and their distance is the reads'.
NEAR_AT = (1160, 1223, 1280, 1655)
ORIENT_D = (0, 1, 60, 300, 849, 850, 851)
ORIENTS = {"FR": (False, True), "RF": (True, False), "FF": (False, False), "RR": (True, True)}  # (left mate minus, right mate minus)
DOVETAILS = (1, 10, 149)
BALLAST_TAIL, BALLAST_TAIL_SEED = 64, 8882
# the choice sequence: seven groups 2 400 bases apart, each with a 150-base locus of its own (kind 0), its copies with 2 and 4
# substitutions, an anchor locus A before the copies and an anchor locus B behind them (offsets from the group's base).  The mate
# at the copies is the locus with MATE_SUBS: they break every 24-mer that only the locus itself holds (the ones that span a
# substitution of either copy), so no seed of the mate is unique and the seed loop cannot settle the pair.
LOCUS_LEN = 150
COPY_SUBS = {0: (), 2: (40, 110), 4: (5, 30, 75, 120)}
MATE_SUBS = (35, 72, 115)
CHOICE_BASE, CHOICE_STEP = 1200, 2400
CHOICE_GROUPS = (
    (0, ((400, 4), (1300, 0)), 1800),           # from A: the worst copy within the limit, the locus beyond it
    (0, ((250, 0), (500, 2)), 1000),            # two within, different scores
    (0, ((250, 2), (500, 0)), 1000),            # the same in the other order
    (0, ((250, 0), (500, 0)), 1000),            # two exact copies within
    (0, ((250, 4), (500, 0), (750, 2)), 1000),  # three within
    (0, ((250, 2), (500, 4), (750, 0)), 1000),  # three within, another order
    (0, ((400, 2), (1300, 0)), 1800),           # from A: the 2-substitution copy within, the locus beyond
)


def store(seed=9201, tail_seed=BALLAST_TAIL_SEED):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for name, n in SEQS:
        s = el._rnd(rng, n)
        if name == "choice":
            for gi, (_, copies, _) in enumerate(CHOICE_GROUPS):
                locus = el._rnd(rng, LOCUS_LEN)
                for at, kind in copies:
                    at += CHOICE_BASE + gi * CHOICE_STEP
                    s[at:at + LOCUS_LEN] = _with_subs(locus, COPY_SUBS[kind])
        if name == "ballast":
            s[n - BALLAST_TAIL:] = el._rnd(np.random.Generator(np.random.PCG64(77000 + tail_seed)), BALLAST_TAIL)
        out.append((name, s))
    return out


def _with_subs(s, at):
    s = s.copy()
    for p in at:
        s[p] = el._sub(s[p])
    return s


def even_subs(L, n):
    """n evenly spaced positions of an L-base mate (in the store's orientation)"""
    return tuple((k + 1) * L // (n + 1) for k in range(n))


def distance_ds(Ll, Lr):
    """the d of one distance series, ascending: around the TL limit, around TLEN = 1000, and the scan windows' ends"""
    half = (Ll + Lr) // 2
    ds = set(range(996 - half, 1005 - half)) | set(range(996 - Lr, 1005 - Lr))
    ds |= {1023 - Lr, 1024 - Lr, 1025 - Lr, 1023, 1024, 1025, 1500}
    return sorted(ds)


class _Builder:
    def __init__(self, st):
        self.store = st
        self.offs, _ = el.layout(st)
        self.reads, self.tags = [], []

    def mate(self, si, pos, L, minus, subs):
        seq = self.store[si][1]
        assert 0 <= pos and pos + L <= len(seq), (si, pos, L)
        s = _with_subs(seq[pos:pos + L], subs)
        return synth.revcomp(s) if minus else np.ascontiguousarray(s)

    def add(self, a, b, flip, **tag):
        """a, b: (sequence index, coordinate, length, minus, substitution positions) of the left and the right mate (None: a random
        partner); flip: b is mate 1"""
        m = []
        for x in (a, b):
            if x is None:
                m.append((tag.pop("partner"), None))
            else:
                si, pos, L, minus, subs = x
                m.append((self.mate(si, pos, L, minus, subs), {"seq": si, "coord": pos, "g": self.offs[si] + pos, "minus": minus, "nsub": len(subs), "len": L}))
        if flip:
            m.reverse()
        k = len(self.tags)
        lab = "{}_{}_d{}_s{}_n{}".format(tag["family"], tag["orient"], tag["d"], tag["nsub"], k)
        self.reads += [(lab + "/1", m[0][0], el._q(len(m[0][0]))), (lab + "/2", m[1][0], el._q(len(m[1][0])))]
        tag.update(flip=flip, Lf=len(m[0][0]), Lr=len(m[1][0]), m1=m[0][1], m2=m[1][1])
        self.tags.append(tag)


def cases(seed=9202, st=None):
    """-> (store, interleaved reads, one tag per pair)"""
    st = st or store()
    rng = np.random.Generator(np.random.PCG64(seed))
    B = _Builder(st)
    A, Bq = SEQ_INDEX["geoA"], SEQ_INDEX["geoB"]
    k = 0
    # distance
    for li, (Ll, Lr) in enumerate(LENGTH_PAIRS):
        for di, d in enumerate(distance_ds(Ll, Lr)):
            for ni, nsub in enumerate(LOADS):
                k += 1
                x = 1100 + (37 * k) % 2000
                B.add((A if li % 2 == 0 else Bq, x, Ll, False, even_subs(Ll, nsub)), (A if li % 2 == 0 else Bq, x + d, Lr, True, even_subs(Lr, nsub)),
                      bool((di + ni + li) & 1), family="distance", orient="FR", d=d, nsub=nsub, series=(Ll, Lr, nsub))
    # the series only the seed loop settles: 56 of the short mate's 64 bases (under its 90 %) beside an exact long mate
    for xi, x in enumerate(NEAR_AT):
        for di, d in enumerate(range(841, 847)):
            B.add((Bq, x, 64, False, NEAR_SUBS), (Bq, x + d, 250, True, ()), bool((xi + di) & 1), family="distance", orient="FR", d=d, nsub=2,
                  series=(64, 250, "near", x))
    # orientation
    for li, (Ll, Lr) in enumerate(((150, 150), (250, 100))):
        for oi, (orient, (lm, rm)) in enumerate(ORIENTS.items()):
            for di, d in enumerate(ORIENT_D):
                for ni, nsub in enumerate((0, 5)):
                    k += 1
                    x = 1100 + (41 * k) % 2000
                    si = Bq if li % 2 == 0 else A
                    B.add((si, x, Ll, lm, even_subs(Ll, nsub)), (si, x + d, Lr, rm, even_subs(Lr, nsub)), bool((di + ni + oi) & 1),
                          family="orientation", orient=orient, d=d, nsub=nsub, series=(Ll, Lr, nsub))
    for di, d in enumerate(DOVETAILS):
        for ni, nsub in enumerate((0, 5)):
            for flip in (False, True):
                k += 1
                x = 1300 + (41 * k) % 2000
                B.add((A, x, 150, True, even_subs(150, nsub)), (A, x + d, 150, False, even_subs(150, nsub)), flip,
                      family="orientation", orient="dovetail", d=d, nsub=nsub, series=(150, 150, nsub))
    # neighbours
    n1 = SEQ_INDEX["nb1"]
    for si in (n1, n1 + 1, n1 + 2):
        n = len(st[si][1])
        for ei, e in enumerate((0, 1, 20, 150)):
            for bi, b in enumerate((0, 1, 10)):
                for flip in (False, True):
                    k += 1
                    nsub = LOADS[k % 3]
                    B.add((si, n - 150 - e, 150, False, even_subs(150, nsub)), (si + 1, b, 150, True, even_subs(150, nsub)), flip,
                          family="neighbours", orient="FR", d=150 + e + PAD + b, nsub=nsub, series="adjacent")
        # the other way round: the mate lower in the store has the lower coordinate
        for lo, hi in ((0, 200), (5, 230), (60, 150)):
            for flip in (False, True):
                k += 1
                nsub = LOADS[k % 3]
                B.add((si, lo, 150, False, even_subs(150, nsub)), (si + 1, hi, 150, True, even_subs(150, nsub)), flip,
                      family="neighbours", orient="FR", d=n - lo + PAD + hi, nsub=nsub, series="adjacent_low_first")
    s4, sl = SEQ_INDEX["nb4"], SEQ_INDEX["nbL"]
    for e in (0, 1, 20):
        for deep in (600, 1200):
            for flip in (False, True):
                k += 1
                nsub = LOADS[k % 3]
                B.add((s4, 400 - 150 - e, 150, False, even_subs(150, nsub)), (sl, deep, 150, True, even_subs(150, nsub)), flip,
                      family="neighbours", orient="FR", d=150 + e + PAD + deep, nsub=nsub, series="short_long")
    for d in (200, 849, 850):
        for flip in (False, True):
            for nsub in (0, 5):
                B.add((sl, 0, 150, False, even_subs(150, nsub)), (sl, d, 150, True, even_subs(150, nsub)), flip,
                      family="neighbours", orient="FR", d=d, nsub=nsub, series="coord0")
    # choice
    ci = SEQ_INDEX["choice"]
    for gi, (a_at, copies, b_at) in enumerate(CHOICE_GROUPS):
        base = CHOICE_BASE + gi * CHOICE_STEP
        a_at, b_at = base + a_at, base + b_at
        exact = base + [at for at, kind in copies if kind == 0][0]  # the mate is the locus with 3 substitutions of its own: every copy is a hit
        for ni, nsub in enumerate((5, 2, 0)):
            for flip in (False, True):
                B.add((ci, a_at, 150, False, even_subs(150, nsub)), (ci, exact, 150, True, MATE_SUBS), flip,
                      family="choice", orient="FR", d=exact - a_at, nsub=nsub, series=("A", gi), group=gi)
                B.add((ci, exact, 150, False, MATE_SUBS), (ci, b_at, 150, True, even_subs(150, nsub)), not flip,
                      family="choice", orient="FR", d=b_at - exact, nsub=nsub, series=("B", gi), group=gi)
    # lonely
    for i, (pos, minus) in enumerate(((1500, False), (2500, False), (3500, False), (1024, True), (1025, True), (2000, True), (4000, True),
                                      (300, True), (700, True), (1000, True), (1023, True), (0, True))):
        k += 1
        partner = el._rnd(rng, 150)
        x = (A, pos, 150, minus, even_subs(150, (0, 2)[i & 1]))
        flip = bool(i & 1)
        B.add(*((x, None) if not minus else (None, x)), flip, family="lonely", orient="-" if minus else "+", d=pos, nsub=(0, 2)[i & 1], series="lonely",
              partner=partner)
    return st, B.reads, B.tags


def read_slots(reads):
    """the index slots of every W-mer of every read, both strands"""
    out = []
    for _, s, _ in reads:
        for t in (s, synth.revcomp(s)):
            v, ok = el.KmerTable.words(t)
            out.append(el.slot_of(v[ok]))
    return np.unique(np.concatenate(out))


def tail_is_clear(st, reads, margin=BALLAST_TAIL - W):
    """no W-mer of a read shares its slot with one of the store's last `margin` W-mers"""
    sd = el.store_bytes(st)
    v, ok = el.KmerTable.words(sd[len(sd) - margin - W + 1:])
    return ok.all() and not np.isin(el.slot_of(v), read_slots(reads)).any()


def find_tail_seed(limit=100000):
    """the smallest BALLAST_TAIL_SEED whose tail is clear of the reads' slots (run when the case lists change)"""
    _, reads, _ = cases()
    rs = read_slots(reads)
    for t in range(limit):
        tail = el._rnd(np.random.Generator(np.random.PCG64(77000 + t)), BALLAST_TAIL)
        v, ok = el.KmerTable.words(tail)
        if not np.isin(el.slot_of(v), rs).any():
            return t
    raise RuntimeError("no clear tail")


# ---------------------------------------------------------------------------------------------------------------------------
# the plain restatement: the TL test and SetSAM2 from the tags alone (shares no code with the oracle or the product)
# ---------------------------------------------------------------------------------------------------------------------------
def tl_within(tag):
    """the reference's limit, as the seed loop, the 90 % shortcut and FindPairs apply it: store positions, integer half-sum"""
    return abs(tag["m1"]["g"] - tag["m2"]["g"]) + (tag["Lf"] + tag["Lr"]) // 2 <= MAX_TL


def expected_sam(tag):
    """((FLAG, RNEXT is '=', PNEXT, TLEN) of mate 1, the same of mate 2) when both mates map where their tags say: coordinates inside
    the sequences, the length of whichever mate has the higher coordinate, 0x2 for 0 < TLEN < 1000 on opposite strands, TLEN
    zeroed only above 1000, PNEXT the mate's POS but 0 for a mate at a sequence's first base"""
    m1, m2 = tag["m1"], tag["m2"]
    if m1["coord"] <= m2["coord"]:
        t = m2["coord"] + tag["Lr"] - m1["coord"]
        sign = 1
    else:
        t = m1["coord"] + tag["Lf"] - m2["coord"]
        sign = -1
    proper = 0 < t < 1000 and m1["minus"] != m2["minus"]
    if t > 1000:
        t = 0
    f1 = 0x41 | (0x10 if m1["minus"] else 0) | (0x20 if m2["minus"] else 0) | (2 if proper else 0)
    f2 = 0x81 | (0x10 if m2["minus"] else 0) | (0x20 if m1["minus"] else 0) | (2 if proper else 0)
    same = m1["seq"] == m2["seq"]
    pnext = lambda m: m["coord"] + 1 if m["coord"] else 0
    return (f1, same, pnext(m2), sign * t), (f2, same, pnext(m1), -sign * t)
