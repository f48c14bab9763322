"""numpy restatement of the reference's index statistics (ufistats.cpp, ufindex.cpp CountSlots / CountSlots_Minus / CountIndexedWords /
GetCollisionCount / GetRow) and of the report LogStats writes.  Used by tests/test_ufi_stats_cpu.py against the reference's fixture and by
the GPU tests against the device passes."""
import gzip
import os
import struct

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TALLY_FREE, TALLY_END, TALLY_PLUS1, TALLY_BOTH1, TALLY_LONG_MINE, TALLY_LONG_OTHER = 0, 127, 254, 255, 253, 125
SAT_EXTRA = "A" * 600 + "GATTACA" * 30 + "CA" * 400  # tests/golden/sat.fa = g.fa + this sequence

_LETTER = np.full(256, 4, dtype=np.uint8)
for _c, _l in zip(b"ACGTUacgtu", (0, 1, 2, 3, 3, 0, 1, 2, 3, 3)):
    _LETTER[_c] = _l


def gunzip(name, d):
    p = os.path.join(d, name[:-3])
    with gzip.open(os.path.join(GOLD, name), "rb") as z, open(p, "wb") as f:
        f.write(z.read())
    return p


class Ufi:
    """a .ufi file's header, slot table and sequence store (ufindexio.cpp:51-115)"""

    def __init__(self, path):
        b = open(path, "rb").read()
        magic, self.W, self.max_ix, self.sds, self.slots, nseq = struct.unpack_from("<IIIIQI", b, 0)
        o = 28
        for _ in range(nseq):
            _, _, n = struct.unpack_from("<III", b, o)
            o += 12 + n
        o += 4
        blob = np.frombuffer(b, dtype=np.uint8, count=5 * self.slots, offset=o).reshape(-1, 5)
        self.tally = blob[:, 0].copy()
        self.pos = blob[:, 1:].copy().view("<u4").ravel()
        o += 5 * self.slots + 4
        self.seq = np.frombuffer(b, dtype=np.uint8, count=self.sds, offset=o)

    def get_row(self, slot):
        """UFIndex::GetRow (ufindex.cpp:776-832)"""
        T = int(self.tally[slot])
        if not T & 0x80:
            return []
        row, s = [], slot
        while True:
            T, pos = int(self.tally[s]), int(self.pos[s])
            row.append(pos)
            if T in (TALLY_PLUS1, TALLY_BOTH1) or len(row) == self.max_ix or T == TALLY_END:
                return row
            if T in (TALLY_LONG_MINE, TALLY_LONG_OTHER):
                a = (s + (pos & 0xFFFF)) % self.slots
                s = (a + (pos >> 16)) % self.slots
                row[-1] = int(self.pos[a])
            else:
                s = (s + (T & 127)) % self.slots
            assert len(row) < 256


def murmur64(h):
    h = h.astype(np.uint64)
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xc4ceb9fe1a85ec53)
        h ^= h >> np.uint64(33)
    return h


def windows(u):
    """the complete words of [0, SeqDataSize - 1): (start positions, plus words, minus words, minus valid)"""
    E, W = u.sds - 1, u.W
    s = u.seq[:E]
    L = _LETTER[s].astype(np.uint64)
    bad = np.concatenate([[0], np.cumsum(L > 3)])
    cbad = np.concatenate([[0], np.cumsum((L > 3) | (s == ord("u")))])
    starts = np.arange(0, max(E - W + 1, 0), dtype=np.int64)
    ok = bad[starts + W] == bad[starts]
    starts = starts[ok]
    fwd = np.zeros(len(starts), dtype=np.uint64)
    rev = np.zeros(len(starts), dtype=np.uint64)
    for i in range(W):
        li = L[starts + i]
        fwd = (fwd << np.uint64(2)) | li
        rev |= (np.uint64(3) - li) << np.uint64(2 * i)
    return starts, fwd, rev, cbad[starts + W] == cbad[starts]


def slot_counts(u):
    """CountSlots and CountSlots_Minus: (plus, minus), uint8 per slot, saturated at 255"""
    _, fwd, rev, rok = windows(u)
    N = np.uint64(u.slots)
    plus = np.bincount((murmur64(fwd) % N).astype(np.int64), minlength=u.slots)
    minus = np.bincount((murmur64(rev[rok]) % N).astype(np.int64), minlength=u.slots)
    return np.minimum(plus, 255).astype(np.uint8), np.minimum(minus, 255).astype(np.uint8)


def stats(u):
    """every number of LogStats's report, as the dict urmap_amd.api.Index.stats() returns"""
    starts, fwd, _, _ = windows(u)
    slot = (murmur64(fwd) % np.uint64(u.slots)).astype(np.int64)
    plus, minus = slot_counts(u)
    rows = {}
    K = np.zeros(u.slots, dtype=np.int64)
    collision = 0
    seq = u.seq.tobytes()
    for s in np.flatnonzero(u.tally & 0x80):
        r = u.get_row(int(s))
        rows[int(s)] = set(r)
        K[s] = len(r)
        w0 = seq[r[0]:r[0] + u.W]
        collision += sum(seq[p:p + u.W] != w0 for p in r[1:])
    indexed = sum(int(p) in rows.get(int(sl), ()) for p, sl in zip(starts, slot))
    t = u.tally
    n, nm = plus.astype(np.int64), minus.astype(np.int64)
    trunc = (n > 0) & (K < n) & (n <= u.max_ix) & (nm <= u.max_ix)
    return {
        "word_length": u.W, "max_ix": u.max_ix, "seqdata_size": u.sds, "slots": u.slots,
        "indexed": indexed, "not_indexed": len(starts) - indexed, "wildcard": (u.sds - 1) - len(starts), "indexed2": int(K.sum()),
        "free": int((t == TALLY_FREE).sum()), "collision": int(collision), "single_both": int((t == TALLY_BOTH1).sum()),
        "single_plus": int((t == TALLY_PLUS1).sum()), "end": int((t == TALLY_END).sum()), "mine": int((t >= 128).sum()),
        "other": int(((t != 0) & (t < 128)).sum()), "trunc": int(n[trunc].sum()), "trunc2": int(trunc.sum()),
        "long_mine": int((t == TALLY_LONG_MINE).sum()), "long_other": int((t == TALLY_LONG_OTHER).sum()), "total": int(n.sum()),
        "count_hist": np.bincount(n, minlength=256).tolist(), "trunc_hist": np.bincount(n[trunc], minlength=256).tolist(),
    }


def int_to_str(x, big=100e6):
    """IntToStr (myutils.cpp:1420-1438); big=10e6: Int64ToStr (1440-1458)"""
    d = float(x)
    if x < 10000:
        return "%u" % x
    if d < 1e6:
        return "%.1fk" % (d / 1e3)
    if d < big:
        return "%.1fM" % (d / 1e6)
    if d < 1e9:
        return "%.0fM" % (d / 1e6)
    if d < 10e9:
        return "%.1fG" % (d / 1e9)
    if d < 100e9:
        return "%.0fG" % (d / 1e9)
    return "%.3g" % d


def mem_bytes_to_str(x):
    """MemBytesToStr (myutils.cpp:1220-1235)"""
    x = float(x)
    for lim, div, fmt in ((1e4, 1, "%.1fb"), (1e6, 1e3, "%.1fkb"), (10e6, 1e6, "%.1fMb"), (1e9, 1e6, "%.0fMb"), (100e9, 1e9, "%.1fGb")):
        if x < lim:
            return fmt % (x / div)
    return "%.0fGb" % (x / 1e9)


def report(st):
    """LogStats's histogram rows and summary block (ufistats.cpp:62-123), as lines"""
    pct = lambda x, y: 100.0 * x / y if y else 0.0
    ch_all, th_all, mx = st["count_hist"], st["trunc_hist"], st["max_ix"]
    maxi = min(4, max([i for i in range(256) if ch_all[i]] or [0]))
    out = []
    for i in range(maxi + 1):
        ch, th = ch_all[i], th_all[i]
        l = "[%3u]  %10u" % (i, ch)
        l += "  %7.7s " % "" if i == 0 else "  %7.2f%%" % pct(ch, st["total"])
        if (1 < i <= mx) or th:
            l += "  %10u  " % th + "  %7.2f%%" % pct(th, ch)
            if i == 1 and th:
                l += " <<< TRUNCATED SINGLES"
            if th and i > mx:
                l += " <<< GT MaxIx %u" % mx
        out.append(l)
    out.append("")
    out.append("%10u  Word length" % st["word_length"])
    out.append("%10u  MaxIx" % mx)
    out.append("%10u  Sequence data (%s)" % (st["seqdata_size"], int_to_str(st["seqdata_size"])))
    out.append("%10u  Slots (%s)" % (st["slots"], int_to_str(st["slots"], 10e6)))
    for name, key in (("Indexed", "indexed"), ("Indexed2", "indexed2"), ("NotIndexed", "not_indexed"), ("Wildcard", "wildcard"),
                      ("Free", "free"), ("Collision", "collision"), ("SingleBoth", "single_both"), ("SinglePlus", "single_plus"),
                      ("End", "end"), ("Mine", "mine"), ("Other", "other"), ("Trunc", "trunc"), ("Trunc2", "trunc2"),
                      ("LongMine", "long_mine"), ("LongOther", "long_other"), ("Total", "total")):
        out.append("%10u  %s" % (st[key], name))
    out.append("")
    return out


def info_lines(u):
    """-ufi_info's four lines (ufistats.cpp:169-173)"""
    return [" Word length  %u" % u.W, "       MaxIx  %u" % u.max_ix, "     SeqData  %u (%s)" % (u.sds, mem_bytes_to_str(u.sds)),
            "       Slots  %u (%s)" % (u.slots, mem_bytes_to_str(u.slots))]


def log_report(text):
    """the histogram rows and the summary block of a -ufi_stats log file, verbatim"""
    lines = text.split("\n")
    hist = [l for l in lines if l.startswith("[") and l[1:4].strip().isdigit() and l[4:7] == "]  "]
    i = next(k for k, l in enumerate(lines) if l.endswith("  Word length"))
    j = next(k for k, l in enumerate(lines) if l.endswith("  Total"))
    return hist + lines[i - 1:j + 2]
