"""-ufi_stats's device passes (ufi_stats.hip) at the headline scale: a 3.1 Gbp genome, 5 392 814 809 slots (more than 2^32), the index
built once by the product's own passes as in test_gpu_fullscale.py.  The counters are checked against what the table and the genome
say on the host: tally classes by bincount, the report's identities, Indexed2 against the validate pass, the plus counts against Total,
and words sampled on the host hashing to slots whose count is at least 1.  URMAP_TEST_FULLSCALE_MBP shrinks the genome (rehearsals on
a small box); the assertions about 2^32 then do not apply."""
import os

import numpy as np
import pytest

import ufistats_lib as U

pytestmark = pytest.mark.gpu

MBP = float(os.environ.get("URMAP_TEST_FULLSCALE_MBP", 3100))
FULL = MBP >= 2600


@pytest.fixture(scope="module")
def full():
    import torch
    import bench
    from urmap_amd import api, ranks

    dev = torch.device("cuda", 0)
    R = ranks.Ranks().init(torch)
    d_seq, lens, offs, labels, desc = bench.make_genome_torch(torch, 20260101, int(MBP * 1e6), dev)
    slots, _ = bench.default_slot_count(lens, labels)
    index, blob_np, seq_np, d_seq, info = bench.place_index(R, torch, api, dev, d_seq, slots, lens, offs, labels)
    yield {"index": index, "blob": blob_np, "seq": seq_np, "slots": slots}
    index.close()
    del d_seq
    torch.cuda.empty_cache()


def test_stats_at_scale(full):
    idx, blob, n = full["index"], full["blob"], full["slots"]
    st = idx.stats()
    print(f"\nufi_stats passes on {n} slots: position {st['position_seconds']:.3f} s, slot {st['slot_seconds']:.3f} s")
    if FULL:
        assert n == 5392814809
    assert st["bad_rows"] == 0 and st["slots"] == n
    # tally classes against a bincount of the tallies (in pieces: 27 GB of table)
    bc = np.zeros(256, dtype=np.int64)
    step = 1 << 28
    for lo in range(0, n, step):
        bc += np.bincount(np.asarray(blob[5 * lo: 5 * min(n, lo + step): 5]), minlength=256)
    assert st["free"] == bc[U.TALLY_FREE] and st["single_plus"] == bc[U.TALLY_PLUS1] and st["single_both"] == bc[U.TALLY_BOTH1]
    assert st["end"] == bc[U.TALLY_END] and st["long_mine"] == bc[U.TALLY_LONG_MINE] and st["long_other"] == bc[U.TALLY_LONG_OTHER]
    assert st["mine"] == bc[128:].sum() and st["other"] == bc[1:128].sum()
    assert sum(st["count_hist"]) == st["free"] + st["mine"] + st["other"] == n
    assert st["indexed"] + st["not_indexed"] + st["wildcard"] == st["seqdata_size"] - 1
    ok, rep = idx.validate()
    assert ok and st["indexed2"] == rep["positions"]
    assert sum(i * c for i, c in enumerate(st["count_hist"])) == st["total"]

    plus = idx.slot_counts()
    assert int(plus.sum(dtype=np.uint64)) == st["total"]
    if FULL:
        assert np.count_nonzero(plus[1 << 32:]) > 0
    # 10 k complete words sampled on the host: their slots hold a count of at least 1
    seq = np.asarray(full["seq"])
    rng = np.random.default_rng(7)
    W, E = st["word_length"], st["seqdata_size"] - 1
    starts = rng.integers(0, E - W, 40000)
    win = seq[starts[:, None] + np.arange(W)[None, :]]
    L = U._LETTER[win].astype(np.uint64)
    good = (L < 4).all(axis=1)
    starts, L = starts[good][:10000], L[good][:10000]
    assert len(starts) == 10000
    w = np.zeros(len(starts), dtype=np.uint64)
    for i in range(W):
        w = (w << np.uint64(2)) | L[:, i]
    slot = (U.murmur64(w) % np.uint64(n)).astype(np.int64)
    assert (plus[slot] >= 1).all()
