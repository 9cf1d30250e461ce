"""The evaluation record's reduce kernel on its own (csrc/kernels/eval_record.hip
eval_record_reduce through csrc/bind_eval_record.cpp), no model in front of it:
the histogram chunk loop (4096 bins at a time) at one, two and three chunks, the
256-thread strided loops at their edges, 64-bit sums, accumulate and reset.

Expected bins are sparse_lr_eval_reference.bins_of over its thresholds, which
is the kernel's tf_threshold_bin rule; everything is compared exactly: the row
losses are multiples of 2^-10 below 2^10, so their fp64 sum is exact in any
order."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sparse_lr_eval_reference as R  # noqa: E402
from eval_record_util import SENT, _record  # noqa: E402

pytestmark = pytest.mark.gpu
BIG = 2 ** 31 - 1
# every T at B = 257; every B at T = 4096 (4097 bins: a second chunk of one bin)
CASES = [(T, 257) for T in (2, 200, 4095, 4096, 8192)] + [(4096, B) for B in (1, 255, 256, 1000)]


def _rows(T, B, seed):
    """(lrow, prow, brow, labels) as NumPy arrays.  prow: 2, NaN, -1, 0, 0.5, 1,
    then every threshold and both its fp32 neighbours in a seeded order, cut (or
    repeated) to B values."""
    rng = np.random.default_rng(seed)
    t = R.thresholds(T).astype(np.float32)
    near = np.concatenate([t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))])
    special = np.array([2.0, np.nan, -1.0, 0.0, 0.5, 1.0], np.float32)
    prow = np.resize(np.concatenate([special, rng.permutation(near)]), B).astype(np.float32)
    labels = rng.choice(np.array([0.0, 1.0, 0.5, -0.0], np.float32), B)
    lrow = (rng.integers(0, 2 ** 20, B) * 2.0 ** -10).astype(np.float32)
    brow = rng.integers(0, 4, B).astype(np.int32)
    brow[[0, B - 1]] = BIG                                  # the sum of two of them needs 64 bits
    return lrow, prow, brow, labels


def _want(T, lrow, prow, brow, labels, times=1):
    k = R.bins_of(prow, T)
    positive = labels != 0                                  # -0.0 is zero
    ls = np.array([times * lrow.astype(np.float64).sum()])
    return (int(ls.view(np.int64)[0]), times * lrow.size, times * int(brow.astype(np.int64).sum()),
            times * np.bincount(k[positive], minlength=T + 1), times * np.bincount(k[~positive], minlength=T + 1))


def _check(big, rec, T, want):
    h = rec.cpu().numpy()
    nb = T + 1
    assert int(big[0]) == SENT and int(big[-1]) == SENT                           # nothing outside the record
    assert (int(h[0]), int(h[1]), int(h[2])) == want[:3]                          # loss-sum bits, rows, bad ids
    assert np.array_equal(h[3:3 + nb], want[3]) and np.array_equal(h[3 + nb:], want[4])


@pytest.mark.parametrize("T,B", CASES)
def test_reduce_exact(native, T, B):
    rows = _rows(T, B, seed=T + B)
    if B == 1000:
        assert R.bins_of(rows[1], T).max() == T and len(np.unique(R.bins_of(rows[1], T))) > 900
    lrow, prow, brow, labels = (torch.from_numpy(a).cuda() for a in rows)
    once, twice = _want(T, *rows), _want(T, *rows, times=2)
    assert once[1] == B and once[2] >= (BIG if B == 1 else 2 * BIG) and once[3].sum() + once[4].sum() == B
    big, rec = _record(T)                                   # prefilled with SENT, garbage loss bits included
    native.eval_record_reduce(lrow, prow, brow, labels, rec, True)
    _check(big, rec, T, once)
    native.eval_record_reduce(lrow, prow, brow, labels, rec, False)
    _check(big, rec, T, twice)
    rec.zero_()
    for _ in range(2):
        native.eval_record_reduce(lrow, prow, brow, labels, rec, False)
    _check(big, rec, T, twice)
    native.eval_record_reduce(lrow, prow, brow, labels, rec, True)
    _check(big, rec, T, once)


def test_refusals_launch_nothing(native):
    T, B = 200, 16
    lrow, prow, brow, labels = (torch.from_numpy(a).cuda() for a in _rows(T, B, seed=0))
    big, rec = _record(T)
    short = [torch.full((n,), SENT, dtype=torch.int64, device="cuda") for n in (7, 8)]
    none = torch.zeros(0, device="cuda")
    bad_calls = [
        (lrow.double(), prow, brow, labels, rec),                                 # a wrong dtype
        (lrow, prow, brow.long(), labels, rec),
        (lrow, prow, brow, labels, rec.int()),
        (lrow, prow.cpu(), brow, labels, rec),                                    # a CPU tensor
        (lrow, prow, brow, labels, rec.cpu()),
        (lrow, prow, brow, labels[:-1].contiguous(), rec),                        # unequal row counts
        (lrow[:-1].contiguous(), prow, brow, labels, rec),
        (lrow, prow, brow, labels, rec[:-1]),                                     # a record of even length
        (lrow, prow, brow, labels, short[0]),                                     # shorter than 9
        (lrow, prow, brow, labels, short[1]),
        (none, none, none.int(), none, rec),                                      # B = 0
    ]
    for args in bad_calls:
        with pytest.raises(RuntimeError):
            native.eval_record_reduce(*args, True)
    torch.cuda.synchronize()
    assert (big == SENT).all() and all((s == SENT).all() for s in short)
    native.eval_record_reduce(lrow, prow, brow, labels, rec, True)
    assert int(rec[1]) == B
