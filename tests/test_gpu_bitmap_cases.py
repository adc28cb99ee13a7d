"""The crafted bitmap cases of tests/bitmap_cases.py on the GPU: encode_bitmap_kernel through
omr_encode_bitmap_device and omr_encode_bitmap under every set_encode_chunks value a case lists, bit for bit
against the plain model (which tests/test_bitmap_cases_host.py proves, with the mutants each case tells apart
and the kernel's FP64 chain in exact integers); a three-call split summed with bitmap_model.add_mod; and the
sums at the carry through omr_digest_merge_bitmap. The output starts as all ones with a guard ciphertext
behind it, every word that comes back is < q2, and every comparison is exact integer equality."""
import time

import numpy as np
import pytest

import bitmap_cases as BC
import bitmap_model as BM
import product_lib as PL
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu

CASES = BC.cases()
Q2, N2 = BC.Q2, BC.N2
ONES = np.uint64(2**64 - 1)


@pytest.fixture(scope="module")
def det():
    d = A.Detector(PL.keys()[2])  # the real key: the encode uses only the context's tables and scratch
    yield d
    d.close()


def dev_pv(c, lo=0, hi=None):
    """The messages [lo, hi) of the case's pertinency vector, built on the device: zeros and the non-zero rows."""
    import torch
    hi = c.D if hi is None else hi
    d_pv = torch.zeros((max(hi - lo, 1), 2, N2), dtype=torch.int64, device="cuda:0")
    ms = [m for m in sorted(c.msgs) if lo <= m < hi]
    if ms:
        rows = np.stack([c.msgs[m] for m in ms]).view(np.int64)
        d_pv[torch.tensor([m - lo for m in ms], device="cuda:0")] = torch.from_numpy(rows).to("cuda:0")
    return d_pv


def encode_device(det, c, lo=0, hi=None):
    """omr_encode_bitmap_device over the messages [lo, hi) of case c; the output starts as all ones and has a
    guard ciphertext behind it."""
    import torch
    hi = c.D if hi is None else hi
    n_ct = BM.ct_count(c.all)
    d_pv = dev_pv(c, lo, hi)
    out = torch.full((n_ct + 1, 2, N2), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    det.encode_bitmap_device(d_pv.data_ptr() if hi > lo else 0, hi - lo, c.offset + lo, c.all, out.data_ptr())
    det.check()
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    assert (got[n_ct] == ONES).all(), "wrote beyond the last ciphertext"
    return got[:n_ct]


@pytest.mark.parametrize("name,knob", BC.runs())
def test_case(det, name, knob):
    c = CASES[name]
    want = c.expected
    t0 = time.perf_counter()
    det.set_encode_chunks(knob)
    try:
        got_device = encode_device(det, c)
        got_host = None if c.device_only else det.encode_bitmap(c.dense(), c.all, c.offset)
    finally:
        det.set_encode_chunks(0)
    if c.device_only:
        print(f"\n{name} under set_encode_chunks({knob}): {c.D * 2 * N2 * 8 / 2**20:.0f} MiB on the device, "
              f"{(time.perf_counter() - t0) * 1e3:.1f} ms for the buffers, the launch and the download")
    assert got_device.shape == want.shape and int(got_device.max()) < Q2
    assert np.array_equal(got_device, want), (name, "device entry", np.argwhere(got_device != want)[:5])
    if got_host is not None:
        assert int(got_host.max()) < Q2
        assert np.array_equal(got_host, want), (name, "host entry", np.argwhere(got_host != want)[:5])
    touched = {(c.offset + m) // BM.PER_CT for m in c.msgs}
    for ct in range(want.shape[0]):
        assert got_device[ct].any() == (ct in touched)


SPLITS = {  # case -> (knob, three consecutive ranges of its messages)
    "two_planes_one_chunk": (1, ((0, 1), (1, 2), (2, 2))),   # either side of the plane boundary, and nothing
    "run_sums": (0, ((0, 3), (3, 4), (4, 8))),               # the run's exact sums move into add_mod
    "edge_l16383_16384": (0, ((0, 1), (1, 1), (1, 2))),      # the ciphertext boundary
}


@pytest.mark.parametrize("name", list(SPLITS))
def test_three_call_split(det, name):
    c = CASES[name]
    knob, ranges = SPLITS[name]
    total = np.zeros_like(c.expected)
    det.set_encode_chunks(knob)
    try:
        for lo, hi in ranges:
            part = encode_device(det, c, lo, hi)
            assert int(part.max()) < Q2
            total = BM.add_mod(total, part)
    finally:
        det.set_encode_chunks(0)
    assert np.array_equal(total, c.expected)


def test_merge_at_the_carry(det):
    """omr_digest_merge_bitmap twice on a fresh session: 0 + a, then a + b with the word-wise integer sums
    q2 - 1, q2, q2 + 1 and 2 q2 - 2; and in the other order."""
    a, b = BC.merge_pair()
    want = BM.add_mod(a, b)
    assert [int(v) for v in want.reshape(-1)[:4]] == [Q2 - 1, 0, 1, Q2 - 2]
    for first, second in ((a, b), (b, a)):
        with det.digest_session(BC.MERGE_ALL, 0, 20261021, bytes(range(32))) as dg:
            dg.enable_bitmap()
            assert not dg.read_bitmap().any()
            dg.merge_bitmap(first)
            assert np.array_equal(dg.read_bitmap(), first)
            dg.merge_bitmap(second)
            got = dg.read_bitmap()
            assert int(got.max()) < Q2 and np.array_equal(got, want)
            idx, pay = dg.read()
            assert not idx.any() and not pay.any()  # the bitmap's merge touches nothing else
