"""Helpers of the GPU evaluation tests (tests/test_*_eval_gpu.py,
test_eval_record_gpu.py): evaluation records and [B] outputs inside
sentinel-filled buffers, and their read-back.  Not a test module."""
import torch

SENT = -0x5A5A5A5A5A5A5A5


def _record(T):
    """A record inside a sentinel-filled buffer: (whole buffer, the record view)."""
    n = 3 + 2 * (T + 1)
    big = torch.full((n + 2,), SENT, dtype=torch.int64, device="cuda")
    return big, big[1:n + 1]


def _read(rec, T):
    h = rec.cpu()
    nb = T + 1
    return (float(h[:1].view(torch.float64)[0]), int(h[1]), int(h[2]), h[3:3 + nb].numpy().copy(),
            h[3 + nb:].numpy().copy())


def _outs(B):
    big = torch.full((2, B + 2), float("nan"), device="cuda")
    return big, big[0, 1:B + 1], big[1, 1:B + 1]


def _check_sentinels(big_rec, big_out, B):
    assert int(big_rec[0]) == SENT and int(big_rec[-1]) == SENT
    edge = big_out[:, [0, B + 1]].cpu()
    assert torch.isnan(edge).all() and not torch.isnan(big_out[:, 1:B + 1]).any()
