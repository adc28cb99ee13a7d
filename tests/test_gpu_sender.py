"""The sender on the GPU (include/omr_gpu.h "Sender"): omr_sender_gen_clues_device against the CPU entry
bit for bit on the crafted keys of sender_cases.py, mixed tables and both stream kinds, its error path,
omr_clue_open_device against omr_clue_open, and a mixed board through the detector. Every comparison is
exact."""
import numpy as np
import pytest

import product_lib as PL
import retriever as R
import sender_cases as SC
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 2, 63, 64, 65, 257)
FILL = 0x5A5A  # device buffers are filled with this before a call; one spare row behind the clues stays so
INVALID_ARGUMENT = r"failed \(1\)"


def _torch():
    import torch
    return torch


def _dev_u16(rows, cols):
    torch = _torch()
    return torch.full((rows * cols,), np.int16(FILL).item(), dtype=torch.int16, device="cuda:0")


def _host_u16(t, rows, cols):
    return t.cpu().numpy().view(np.uint16).reshape(rows, cols)


def _dev_of(x):
    """A device copy of a numpy array of u8 / u16 / u32 (as the signed torch type of its width)."""
    torch = _torch()
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view({1: np.uint8, 2: np.int16, 4: np.int32}[x.dtype.itemsize])).to("cuda:0")


def _stream(kind):
    torch = _torch()
    return torch.cuda.Stream() if kind == "side" else None


def _gen_device(snd, seed, first, count, rec, st=None):
    """omr_sender_gen_clues_device into FILLed buffers with one spare row; returns the clues (the spare rows
    are asserted untouched)."""
    torch = _torch()
    da, db = _dev_u16(count + 1, 512), _dev_u16(count + 1, 7)
    dr = None if rec is None else _dev_of(rec if count else np.zeros(1, np.uint32))
    torch.cuda.synchronize()
    snd.gen_clues_device(seed, first, count, da.data_ptr(), db.data_ptr(), 0 if dr is None else dr.data_ptr(),
                         st.cuda_stream if st else 0)
    ga, gb = _host_u16(da, count + 1, 512), _host_u16(db, count + 1, 7)
    assert (ga[count] == FILL).all() and (gb[count] == FILL).all(), "wrote past the last clue"
    return ga[:count], gb[:count]


@pytest.mark.parametrize("stream", ["null", "side"])
@pytest.mark.parametrize("first", SC.FIRSTS)
def test_device_clues_equal_the_cpu_entry_on_crafted_keys(first, stream):
    st = _stream(stream)
    for name, key in SC.crafted_keys().items():
        snd = A.Sender(A.ClueKey(*key), device=0)
        for count in COUNTS:
            ea, eb = snd.gen_clues(SC.SEED, first, count, nthreads=16)
            ga, gb = _gen_device(snd, SC.SEED, first, count, None, st)
            assert np.array_equal(ga, ea) and np.array_equal(gb, eb), (name, count)
        snd.close()


@pytest.mark.parametrize("stream", ["null", "side"])
def test_device_three_key_table_follows_the_recipients(stream):
    st = _stream(stream)
    snd = A.Sender(SC.table(("generated", "alternating", "all_2047")), device=0)
    for first in SC.FIRSTS:
        for pattern in SC.RECIPIENT_PATTERNS:
            for count in COUNTS:
                rec = SC.recipients(pattern, count)
                ea, eb = snd.gen_clues(SC.SEED, first, count, rec, nthreads=16)
                ga, gb = _gen_device(snd, SC.SEED, first, count, rec, st)
                assert np.array_equal(ga, ea) and np.array_equal(gb, eb), (first, pattern, count)
    snd.close()


def test_one_key_equal_to_the_packs_key_gives_gen_clues_device_bits():
    torch = _torch()
    pack = SC.packs()[0]
    snd = A.Sender(pack.clue_key(), device=0)
    for first in SC.FIRSTS:
        da, db = _dev_u16(257, 512), _dev_u16(257, 7)
        torch.cuda.synchronize()
        pack.gen_clues_device(SC.SEED, first, 257, da.data_ptr(), db.data_ptr())
        ga, gb = _gen_device(snd, SC.SEED, first, 257, None)
        assert np.array_equal(ga, _host_u16(da, 257, 512)) and np.array_equal(gb, _host_u16(db, 257, 7))
    snd.close()


def test_recipient_out_of_range_names_the_message_and_skips_its_clue():
    """An error path of a clean run: the kernel skips the message whose id is not a key of the table."""
    snd = A.Sender(SC.table(("generated", "alternating", "x1_x6")), device=0)
    count = 65
    good = SC.recipients("alternating", count)
    want = snd.gen_clues(SC.SEED, 7, count, good, nthreads=16)
    rec = good.copy()
    rec[33] = 3  # = n_keys
    torch = _torch()
    da, db, dr = _dev_u16(count + 1, 512), _dev_u16(count + 1, 7), _dev_of(rec)
    torch.cuda.synchronize()
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT + r".*message 33\b"):
        snd.gen_clues_device(SC.SEED, 7, count, da.data_ptr(), db.data_ptr(), dr.data_ptr())
    ga, gb = _host_u16(da, count + 1, 512), _host_u16(db, count + 1, 7)
    assert (ga[33] == FILL).all() and (gb[33] == FILL).all() and (ga[count] == FILL).all()
    keep = np.arange(count) != 33
    assert np.array_equal(ga[:count][keep], want[0][keep]) and np.array_equal(gb[:count][keep], want[1][keep])
    # two offenders: the smallest index is named; then the sender works as before
    rec[12] = 0xFFFFFFFF
    dr = _dev_of(rec)
    torch.cuda.synchronize()
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT + r".*message 12\b"):
        snd.gen_clues_device(SC.SEED, 7, count, da.data_ptr(), db.data_ptr(), dr.data_ptr())
    ga, gb = _gen_device(snd, SC.SEED, 7, count, good)
    assert np.array_equal(ga, want[0]) and np.array_equal(gb, want[1])
    snd.close()
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):  # a sender without a device has no device entry
        A.Sender(SC.table(("generated",))).gen_clues_device(SC.SEED, 0, 1, da.data_ptr(), db.data_ptr())


# ---- opening ------------------------------------------------------------------------------------------
OUTPUTS = ("values", "pertinent", "max_abs_noise")


def _open_device(pack, ca, cb, ask):
    torch = _torch()
    n = ca.shape[0]
    da, db = _dev_of(ca), _dev_of(cb)
    bufs = {k: torch.full(((n + 1) * (7 if k == "values" else 1),), 0xEE, dtype=torch.uint8, device="cuda:0") for k in ask}
    torch.cuda.synchronize()
    pack.open_clues_device(da.data_ptr(), db.data_ptr(), n, *[bufs[k].data_ptr() if k in bufs else 0 for k in OUTPUTS])
    out = {}
    for k, t in bufs.items():
        h = t.cpu().numpy()
        w = 7 if k == "values" else 1
        assert (h[n * w:] == 0xEE).all(), "wrote past the last message"
        out[k] = h[:n * w].reshape(n, 7) if k == "values" else h[:n]
    return out


@pytest.mark.parametrize("case", ["crafted_phases", "board"])
def test_open_device_equals_open(case):
    pack = SC.packs()[0]
    if case == "crafted_phases":
        ca, cb, _ = SC.crafted_phase_clues()
    else:
        rec, ca, cb, _ = SC.board()
    want = pack.open_clues(ca, cb, nthreads=16)
    for ask in (OUTPUTS, OUTPUTS[1:], OUTPUTS[:1] + OUTPUTS[2:], OUTPUTS[:2]):  # all, then each output NULL in turn
        got = _open_device(pack, ca, cb, ask)
        assert list(got) == list(ask)
        for k in ask:
            assert np.array_equal(got[k], want[k]), (case, ask, k)
    if case == "board":
        assert np.array_equal(want["pertinent"], rec == 0)
        for n in (1, 3, 4, 5, 16, 17, 19):  # a partial last wave, a partial last workgroup
            got = _open_device(pack, ca[:n], cb[:n], OUTPUTS)
            assert all(np.array_equal(got[k], want[k][:n]) for k in OUTPUTS), n
    da, db = _dev_of(ca), _dev_of(cb)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        pack.open_clues_device(da.data_ptr(), db.data_ptr(), 1)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        pack.open_clues_device(da.data_ptr() + 2, db.data_ptr(), 1, d_pertinent=db.data_ptr())  # not 16-byte aligned


# ---- end to end ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector():
    _torch().cuda.init()
    det = A.Detector(PL.keys()[2], device=0)
    yield det
    det.close()


@pytest.mark.parametrize("D", [96, 5])  # throughput kernels, latency kernels
def test_mixed_board_through_the_detector(detector, D):
    torch = _torch()
    packs = SC.packs()
    snd = A.Sender([p.clue_key() for p in packs], device=0)
    rec = np.random.default_rng(D).integers(0, 3, D).astype(np.uint32)
    rec[:3] = (1, 0, 2)
    da, db, dr = _dev_u16(D, 512), _dev_u16(D, 7), _dev_of(rec)
    dout = torch.zeros(D * 2 * 2048, dtype=torch.int64, device="cuda:0")
    dpert = torch.zeros(D, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    snd.gen_clues_device(SC.SEED + 2, 1000, D, da.data_ptr(), db.data_ptr(), dr.data_ptr())
    packs[0].open_clues_device(da.data_ptr(), db.data_ptr(), D, d_pertinent=dpert.data_ptr())
    detector.detect_batch_device(da.data_ptr(), db.data_ptr(), D, dout.data_ptr())
    detector.check()
    pv = dout.cpu().numpy().view(np.uint64).reshape(D, 2, 2048)
    s2 = packs[0].export()["s2"]
    found = np.zeros(D, bool)
    for m in range(D):
        d = R.decrypt_decode(s2, pv[m])
        if rec[m] == 0:
            assert d[0] == 1 and not d[1:].any(), m
            found[m] = True
        else:
            assert not d.any(), m
    assert np.array_equal(found, rec == 0)
    assert np.array_equal(dpert.cpu().numpy().astype(bool), found)
    snd.close()
