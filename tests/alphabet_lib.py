"""Seeded reads and mates in tagged letter classes (test infrastructure; numpy only).

The search kernels have different code for different letters: a read of upper-case ACGT only takes the fast complement / code and
two bit planes ("plain"), a read with N or lower case takes the general functions and four planes ("four"), a read with any other
letter is compared as ASCII ("other", the kernels' q_other).  The reference's FASTQ reader accepts every isalpha byte
(fastqseqsource.cpp:78); U / u hash as T; u and E F I J L O P Q Z have no complement and become '?' on the reverse strand
(alpha.cpp:3005).  The classes below put each of these into reads and, independently, into the two mates of a pair.

Reads are cut from the sequence store AS THE INDEX HOLDS IT: class `case_kept` keeps its bytes, so that an N of a read has to
MATCH the store's N -- and, on an index whose store kept the FASTA's case (soft_masked_index), a lower-case letter the store's.
Every read carries a tag dict: cls, kind, seq_index, coord (0-based, leftmost base), plus, subs (None: sub/indel model), lower
(the window overlaps a lower-cased stretch), n_edge (it touches the edge of an N run), unique (every 24-mer of the window occurs
once in the store, either strand: the read lies outside the repeat families).
"""
from __future__ import annotations

import numpy as np

from urmap_amd import synth

CLASSES = ("plain", "n_mid", "n_first", "n_last", "n_run", "all_n", "lower_all", "lower_stretch", "iupac_upper", "iupac_lower",
           "U_for_T", "u_for_t", "no_complement", "case_kept")
KINDS = ("plain", "four", "other")
IUPAC = np.frombuffer(b"RYKMSWBDHVX", np.uint8)
NO_COMP = np.frombuffer(b"EFIJLOPQZefijlopqz", np.uint8)
ALL_LETTERS = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz", np.uint8)
W = 24

_FOUR = np.zeros(256, bool)
_FOUR[list(b"ACGTNacgtn")] = True
_PLAIN = np.zeros(256, bool)
_PLAIN[list(b"ACGT")] = True


def kind_of(seq: np.ndarray) -> str:
    """which set-up of the search kernels a read or mate takes"""
    if _PLAIN[seq].all():
        return "plain"
    return "four" if _FOUR[seq].all() else "other"


def fasta_lower_masks(fasta):
    """per sequence of a FASTA file: bool per base, True where the file has a lower-case letter (a soft-masked stretch)"""
    out, cur = [], None
    with open(fasta, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                cur = []
                out.append(cur)
            elif cur is not None:
                b = np.frombuffer(line.strip(), np.uint8)
                cur.append((b & 0x20) != 0)
    return [np.concatenate(c) if c else np.zeros(0, bool) for c in out]


def soft_masked_index(oracle_index, fasta):
    """-make_ufi upper-cases the FASTA (seqdb.cpp:983), so no index the reference builds holds a lower-case letter, and a
    lower-case letter of a read never matches.  This is the same index with the FASTA's case put back into the sequence store (the
    slot table hashes case-blind and stays as it is): on it a read that keeps the store's case has to match lower case against
    lower case -- the store-side codes 5..9 of the kernels' four-plane compare, which nothing else reaches."""
    import oracle_lib as ol
    oi = oracle_index
    d = oi.directory()
    sd = oi.seqdata().copy()
    for (lab, ln, off), m in zip(d, fasta_lower_masks(fasta)):
        assert len(m) == ln, (lab, ln, len(m))
        sd[off:off + ln][m] |= 0x20
    blob = np.zeros(5 * oi.slot_count + 16, np.uint8)
    blob[:5 * oi.slot_count] = oi.blob()
    return ol.Index.wrap(oi.word_length, oi.max_ix, oi.slot_count, blob[:5 * oi.slot_count], sd, [x[1] for x in d],
                         [x[2] for x in d], [x[0] for x in d])


class Store:
    """The sequences of an index as the index holds them (oracle_lib.Index: seqdata + directory), and what the generator needs
    to place reads: where the lower-cased stretches (of the FASTA, or of a store that kept case) and the N runs are, which
    windows lie outside the repeat families."""

    def __init__(self, oracle_index, fasta=None):
        sd = oracle_index.seqdata()
        self.seqs = [(lab, np.array(sd[off:off + ln])) for lab, ln, off in oracle_index.directory()]
        self.lower = [(s & 0x20) != 0 for _, s in self.seqs]
        if fasta is not None:
            self.lower = [a | b for a, b in zip(self.lower, fasta_lower_masks(fasta))]
        self._uniq = [None] * len(self.seqs)

    def _kmer_unique(self):
        """per sequence: bool per 24-mer start, True where the 24-mer (case-blind, either strand) occurs once in the store"""
        code = np.full(256, 4, np.uint64)
        for k, c in enumerate(b"ACGT"):
            code[c] = code[c | 0x20] = k
        vals, oks = [], []
        for _, s in self.seqs:
            c = code[s]
            n = len(s) - W + 1
            f = np.zeros(n, np.uint64)
            r = np.zeros(n, np.uint64)
            ok = np.ones(n, bool)
            for j in range(W):
                cj = c[j:j + n]
                ok &= cj < 4
                f |= (cj & np.uint64(3)) << np.uint64(2 * (W - 1 - j))
                r |= ((np.uint64(3) - cj) & np.uint64(3)) << np.uint64(2 * j)
            vals.append(np.minimum(f, r))
            oks.append(ok)
        allv = np.concatenate([v[o] for v, o in zip(vals, oks)])
        u, cnt = np.unique(allv, return_counts=True)
        once = u[cnt == 1]
        for i, (v, o) in enumerate(zip(vals, oks)):
            self._uniq[i] = np.isin(v, once) | ~o  # a 24-mer with an N seeds nothing: it cannot make the window a repeat

    def window_unique(self, si, pos, L):
        if self._uniq[0] is None:
            self._kmer_unique()
        return bool(self._uniq[si][pos:pos + L - W + 1].all())


def _other_base(rng, b):
    acgt = synth.ACGT
    w = np.nonzero(acgt == (b & 0xDF))[0]
    k = int(w[0]) if len(w) else 0
    return acgt[(k + 1 + int(rng.integers(0, 3))) % 4] | (b & 0x20)


def apply_class(rng, s: np.ndarray, cls: str) -> np.ndarray:
    """the letters of class `cls` put into read `s` (upper-case ACGTN on entry; case_kept and plain come back unchanged)"""
    s = s.copy()
    L = len(s)
    if cls in ("plain", "case_kept"):
        return s
    if cls == "n_mid":
        s[int(rng.integers(1, L - 1))] = ord("N")
    elif cls == "n_first":
        s[0] = ord("N")
    elif cls == "n_last":
        s[L - 1] = ord("N")
    elif cls == "n_run":
        n = min(L, W + int(rng.integers(0, 17)))
        p = int(rng.integers(0, L - n + 1))
        s[p:p + n] = ord("N")
    elif cls == "all_n":
        s[:] = ord("N")
    elif cls == "lower_all":
        s |= 0x20
    elif cls == "lower_stretch":
        n = min(L, int(rng.integers(10, 41)))
        p = int(rng.integers(0, L - n + 1))
        s[p:p + n] |= 0x20
    elif cls in ("iupac_upper", "iupac_lower"):
        for p in rng.choice(L, int(rng.integers(1, 4)), replace=False):
            s[p] = IUPAC[int(rng.integers(0, len(IUPAC)))] | (0x20 if cls == "iupac_lower" else 0)
    elif cls in ("U_for_T", "u_for_t"):
        u = ord("U") if cls == "U_for_T" else ord("u")
        t = np.nonzero(s == ord("T"))[0]
        if len(t) == 0:
            s[int(rng.integers(0, L))] = u
        elif rng.random() < 1 / 3:
            s[t] = u
        else:
            s[t[int(rng.integers(0, len(t)))]] = u
    elif cls == "no_complement":
        for p in rng.choice(L, int(rng.integers(1, 4)), replace=False):
            s[p] = NO_COMP[int(rng.integers(0, len(NO_COMP)))]
    else:
        raise ValueError(cls)
    return s


def _n_run_edges(s):
    isn = (s & 0xDF) == ord("N")
    d = np.diff(isn.astype(np.int8))
    return np.nonzero(d == 1)[0] + 1, np.nonzero(d == -1)[0] + 1  # first N of a run, first base after a run


def _place(rng, store: Store, L, how, span):
    """a window of `span` bases whose first L bases are placed as `how` asks: 'lower' (overlaps a lower-cased stretch), 'n_edge'
    (begins or ends a few bases inside an N run), 'any'; outside the repeat families where one is found in 40 draws"""
    best = None
    for _ in range(40):
        si = int(rng.integers(0, len(store.seqs)))
        s = store.seqs[si][1]
        if len(s) < span + 64:
            continue
        pos = None
        if how == "lower":
            low = np.nonzero(store.lower[si])[0]
            if len(low):
                pos = int(low[int(rng.integers(0, len(low)))]) - int(rng.integers(0, L))
        elif how == "n_edge":
            starts, ends = _n_run_edges(s)
            k = int(rng.integers(1, 9))
            if len(ends) and rng.random() < 0.5:
                pos = int(ends[int(rng.integers(0, len(ends)))]) - k  # k N's, then sequence
            elif len(starts):
                pos = int(starts[int(rng.integers(0, len(starts)))]) + k - L  # sequence, then k N's
        else:
            pos = int(rng.integers(0, len(s) - span))
        if pos is None or pos < 0 or pos + span > len(s):
            continue
        w = s[pos:pos + L]
        if ((w & 0xDF) == ord("N")).sum() > 16:
            continue
        best = (si, pos)
        if store.window_unique(si, pos, L):
            break
    if best is None:
        return _place(rng, store, L, "any", span)
    return best


def _tag(store, cls, seq, si, pos, L, plus, subs):
    isn = (store.seqs[si][1][max(0, pos - 1):pos + L + 1] & 0xDF) == ord("N")
    return {"cls": cls, "kind": kind_of(seq), "seq_index": si, "coord": pos, "plus": plus, "subs": subs,
            "lower": bool(store.lower[si][pos:pos + L].any()), "n_edge": bool(isn.any() and not isn.all()),
            "unique": store.window_unique(si, pos, L)}


def _cut(rng, store, cls, si, pos, L, minus, sub, indel):
    """one read of class cls from window (si, pos): case_kept keeps the store's bytes (half of them get one or two
    substitutions), every other class is cut from the upper-cased store with the sub / indel model and then gets its letters"""
    s = store.seqs[si][1]
    if cls == "case_kept":
        r = s[pos:pos + L].copy()
        subs = int(rng.integers(1, 3)) if rng.random() < 0.5 else 0
        for p in rng.choice(L, subs, replace=False):
            if (r[p] & 0xDF) != ord("N"):
                r[p] = _other_base(rng, r[p])
        if minus:
            r = synth.revcomp(r)  # case-preserving on ACGTN
        return r, subs
    frag = s[pos:pos + L + 16] & 0xDF
    frag = np.where(_PLAIN[frag] | (frag == ord("N")), frag, ord("N")).astype(np.uint8)
    r = synth._mutate(rng, frag, sub, indel, indel)[:L]
    if len(r) < L:
        r = np.concatenate([r, synth.ACGT[rng.integers(0, 4, L - len(r))]])
    if minus:
        r = synth.revcomp(r)
    return apply_class(rng, np.ascontiguousarray(r, dtype=np.uint8), cls), None


def _how(k, cls):
    """where the k-th read or mate of its class goes: of ten case_kept reads five on a lower-cased stretch, two on the edge of an
    N run, three anywhere"""
    if cls != "case_kept":
        return "any"
    return ("lower", "n_edge", "lower", "any", "lower", "any", "lower", "n_edge", "lower", "any")[k % 10]


def make_reads(seed, store: Store, n, read_len=150, sub=0.01, indel=0.001, classes=CLASSES, prefix="a"):
    """n reads, the classes in turn -> (reads [(label, seq, qual)], tags).  read_len: an int or (lo, hi) for lengths drawn per read."""
    rng = np.random.Generator(np.random.PCG64(seed))
    reads, tags = [], []
    for i in range(n):
        cls = classes[i % len(classes)]
        L = read_len if isinstance(read_len, int) else int(rng.integers(read_len[0], read_len[1] + 1))
        si, pos = _place(rng, store, L, _how(i // len(classes), cls), L + 16)
        minus = bool(rng.random() < 0.5)
        r, subs = _cut(rng, store, cls, si, pos, L, minus, sub, indel)
        reads.append((f"{prefix}{i}c{classes.index(cls)}", r, np.full(L, ord("I"), np.uint8)))
        tags.append(_tag(store, cls, r, si, pos, L, not minus, subs))
    return reads, tags


def _pair_classes(rng, n, classes):
    """classes of the two mates, independent of each other: a wheel of the classes (plain four times; U_for_T and u_for_t twice,
    since only some of their reads can map) turned by one step per pair for mate 1 and by seven for mate 2, plus one more step
    each time mate 1's wheel has gone round -- every (class, class) combination comes up once in len(wheel)^2 pairs"""
    wheel = ["plain"] * 4 + [c for c in classes if c != "plain"] + [c for c in ("U_for_T", "u_for_t") if c in classes]
    m = len(wheel)
    out = [(wheel[i % m], wheel[(7 * i + i // m) % m]) for i in range(n)]
    return [out[k] for k in rng.permutation(n)]


def make_pairs(seed, store: Store, n, read_len=150, insert_mean=300, insert_sd=50, sub1=0.01, sub2=0.02, indel=0.001,
               classes=CLASSES, prefix="a"):
    """n FR pairs, the class of each mate drawn on its own -> (reads1, reads2, tags1, tags2)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    L = read_len
    r1, r2, t1, t2 = [], [], [], []
    q = np.full(L, ord("I"), np.uint8)
    for i, (c1, c2) in enumerate(_pair_classes(rng, n, classes)):
        isz = int(max(L + 20, rng.normal(insert_mean, insert_sd)))
        flip = bool(rng.random() < 0.5)  # mate 1 is the fragment's reverse-strand end
        ca, cb = (c2, c1) if flip else (c1, c2)  # a: forward strand at the fragment's start, b: reverse strand at its end
        if cb == "case_kept" and ca != "case_kept":  # place the fragment by its case_kept mate's window
            si, pb = _place(rng, store, L, _how(i, cb), L + 16)
            pos = pb - (isz - L)
            if pos < 0:
                si, pos = _place(rng, store, L, "any", isz + 32)
        else:
            si, pos = _place(rng, store, L, _how(i, ca), isz + 32)
        a, sa = _cut(rng, store, ca, si, pos, L, False, sub2 if flip else sub1, indel)
        pb = pos + isz - L
        if cb == "case_kept":
            b, sb = _cut(rng, store, cb, si, pb, L, True, 0, 0)
        else:  # the sub / indel model runs along the read: cut the reverse strand of the fragment's end
            s = store.seqs[si][1]
            lo = max(0, pb - 16)
            frag = synth.revcomp(np.where(_FOUR[s[lo:pb + L]], s[lo:pb + L] & 0xDF, ord("N")).astype(np.uint8))
            m = synth._mutate(rng, frag, sub1 if flip else sub2, indel, indel)[:L]
            if len(m) < L:
                m = np.concatenate([m, synth.ACGT[rng.integers(0, 4, L - len(m))]])
            b, sb = apply_class(rng, np.ascontiguousarray(m, dtype=np.uint8), cb), None
        ta = _tag(store, ca, a, si, pos, L, True, sa)
        tb = _tag(store, cb, b, si, pb, L, False, sb)
        lab = f"{prefix}{i}c{classes.index(c1)}c{classes.index(c2)}"
        (m1, m2, g1, g2) = (b, a, tb, ta) if flip else (a, b, ta, tb)
        r1.append((lab + "/1", m1, q))
        r2.append((lab + "/2", m2, q))
        t1.append(g1)
        t2.append(g2)
    return r1, r2, t1, t2


# ---------------------------------------------------------------------------------------------------------------------------
# conditions that keep a test from passing vacuously, checked on the ORACLE's results alone
# ---------------------------------------------------------------------------------------------------------------------------
UNMAPPED = 0xFFFFFFFF
MIN_PER_CLASS = 20
FREE_CLASSES = ("all_n", "n_run", "lower_all")  # classes that need not map


def class_counts(tags, ores):
    """{class: (reads, mapped)}"""
    mapped = ores["dbpos"] != UNMAPPED
    out = {}
    for t, m in zip(tags, mapped):
        a = out.setdefault(t["cls"], [0, 0])
        a[0] += 1
        a[1] += int(m)
    return {k: tuple(v) for k, v in out.items()}


def case_kept_exact(tags, ores):
    """(reads, of them at their own position with a full-length score) among case_kept reads without substitutions that overlap
    a lower-cased stretch and lie outside the repeat families"""
    n = ok = 0
    for i, t in enumerate(tags):
        if t["cls"] == "case_kept" and t["subs"] == 0 and t["lower"] and t["unique"]:
            n += 1
            r = ores[i]
            L = int(t["len"]) if "len" in t else None
            ok += int(r["dbpos"] != UNMAPPED and int(r["seq_index"]) == t["seq_index"] and int(r["coord"]) == t["coord"]
                      and bool(r["plus"]) == t["plus"] and (L is None or int(r["score"]) == L))
    return n, ok


def check_classes(tags, ores, lens, classes=CLASSES, min_exact=MIN_PER_CLASS):
    """every class except all_n, n_run, lower_all has >= 20 mapped reads (or mates), lower_all >= 20 unmapped; >= 90 % of the
    case_kept reads that have to match lower-case letters do so, full length, at their own position -> the counts, for reports"""
    for t, L in zip(tags, lens):
        t["len"] = int(L)
    cc = class_counts(tags, ores)
    for c in classes:
        n, m = cc.get(c, (0, 0))
        if c == "lower_all":
            assert n - m >= MIN_PER_CLASS, (c, n, m)
        elif c not in FREE_CLASSES:
            assert m >= MIN_PER_CLASS, (c, n, m)
    if "case_kept" in classes:
        n, ok = case_kept_exact(tags, ores)
        assert n >= min_exact and ok >= 0.9 * n, ("case_kept reads on lower-cased stretches, exact at their own position", n, ok)
        assert sum(1 for t in tags if t["cls"] == "case_kept" and t["lower"]) * 3 >= sum(1 for t in tags if t["cls"] == "case_kept")
        assert any(t["cls"] == "case_kept" and t["n_edge"] for t in tags)
        cc["case_kept_exact"] = (n, ok)
    return cc


def check_pair_kinds(t1, t2, sam: bytes):
    """all nine (kind of mate 1, kind of mate 2) combinations with >= 10 pairs each; each non-plain kind in mate 2 alone; >= 30
    proper pairs (FLAG 99 / 83 on mate 1) whose mate 2 is not plain -> {(k1, k2): pairs}, proper pairs with a non-plain mate 2"""
    combos = {}
    for a, b in zip(t1, t2):
        combos[(a["kind"], b["kind"])] = combos.get((a["kind"], b["kind"]), 0) + 1
    for k1 in KINDS:
        for k2 in KINDS:
            assert combos.get((k1, k2), 0) >= 10, (k1, k2, combos)
    recs = [l for l in sam.split(b"\n") if l and not l.startswith(b"@")]
    assert len(recs) == 2 * len(t1), (len(recs), len(t1))
    proper = sum(1 for i in range(len(t1)) if t2[i]["kind"] != "plain" and recs[2 * i].split(b"\t")[1] in (b"99", b"83"))
    assert proper >= 30, proper
    return combos, proper
