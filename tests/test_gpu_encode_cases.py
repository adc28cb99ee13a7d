"""The crafted encode cases of tests/encode_cases.py on the GPU: encode_indices_kernel and the payload kernels
over TableWeights, IndexedWeights and SeekWeights, through the device entry and the host entry of each, bit
for bit against the plain model (which tests/test_encode_cases_host.py pins to the oracle, with the mutants
each case tells apart); the sums at the carry through a digest session's merge and update; and the argument
checks of omr_encode_indices_device.

A session takes clues, not a pertinency vector, so its carry cases steer the other side of the sum: the model
gives the partial of a real update (its pv from omr_detect_batch), and the array merged before it is chosen so
that the running digest plus that partial is, word for word and before any reduction, exactly q2, q2 - 1,
q2 + 1 or a half boundary (encode_cases.steer). Every comparison is exact integer equality."""
import numpy as np
import pytest

import encode_cases as EC
import product_lib as PL
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu

CASES = EC.cases()
INVALID_ARGUMENT = r"failed \(1\)"  # OMR_ERR_INVALID_ARGUMENT in omr_amd._check's message
Q2, N2 = EC.Q2, EC.N2


@pytest.fixture(scope="module")
def det():
    _, _, dk = PL.keys()  # the real key: the encode uses only the context's tables and scratch
    d = A.Detector(dk)
    yield d
    d.close()


def dev(x):
    import torch
    x = np.array(x)  # torch wants a writable array
    return torch.from_numpy(x.view({2: np.int16, 8: np.int64}[x.dtype.itemsize])).to("cuda:0")


def out_buffer(n_ct):
    import torch
    return torch.full((n_ct, 2, N2), -1, dtype=torch.int64, device="cuda:0")


def host_of(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def board_params(c):
    """RetrievalParams of the case's board with the payload layout of the call."""
    rp = A.RetrievalParams(c.all, 0)
    rp.combination_count, rp.cmb_cipher_count, rp.cmb_count_per_cipher = c.combos, c.first_ct + c.n_ct, c.per_ct
    return rp


_SEEKS = {}


def seek_of(c):
    key = (c.seed, c.combos * c.all)
    if key not in _SEEKS:
        _SEEKS[key] = A.WeightSeek.build(*key)
    return _SEEKS[key]


def run_device(det, c):
    d_pv, d_out = dev(c.pv), out_buffer(c.n_ct)
    pv_ptr = d_pv.data_ptr()
    if c.kind == "indices":
        det.encode_indices_device(pv_ptr, c.D, c.offset, c.all, c.seed, c.first_ct, c.n_ct, d_out.data_ptr())
        return host_of(d_out)
    d_pay = dev(c.payloads)
    args = (pv_ptr, d_pay.data_ptr(), c.D, c.offset, c.all)
    if c.kind == "table":
        d_w = dev(c.weights)  # the call's first row: ciphertext first_ct's first combination
        first_row = d_w.data_ptr() + 2 * c.first_ct * c.per_ct * c.all
        det.encode_payloads_device(*args, first_row, c.n_ct, c.per_ct, d_out.data_ptr())
    elif c.kind == "indexed":
        det.encode_pertinent_payloads_indexed_device(*args, c.seed, c.combos, c.first_ct, c.n_ct, c.per_ct,
                                                     d_out.data_ptr())
    else:
        det.encode_pertinent_payloads_seek_device(*args, c.seed, seek_of(c), c.combos, c.first_ct, c.n_ct, c.per_ct,
                                                  d_out.data_ptr())
    return host_of(d_out)


def run_host(det, c):
    rp = board_params(c)
    if c.kind == "indices":
        return np.stack([det.encode_pertinent_indices(rp, c.pv, c.seed, c.first_ct + y, c.offset)
                         for y in range(c.n_ct)])
    if c.kind == "table":
        rp.cmb_cipher_count = c.n_ct
        return det.encode_pertinent_payloads(c.pv, c.payloads, c.weights[c.first_ct * c.per_ct * c.all:], rp, c.offset)
    if c.kind == "indexed":
        return det.encode_pertinent_payloads_indexed(c.pv, c.payloads, c.seed, rp, c.offset, c.first_ct, c.n_ct)
    return det.encode_pertinent_payloads_seek(c.pv, c.payloads, c.seed, seek_of(c), rp, c.offset, c.first_ct, c.n_ct)


@pytest.mark.parametrize("name", list(CASES))
def test_case(det, name):
    c = CASES[name]
    want = c.expected
    det.set_encode_chunks(c.max_chunks)
    try:
        got_device = run_device(det, c)
        got_host = run_host(det, c)
    finally:
        det.set_encode_chunks(0)
    assert np.array_equal(got_device, want), f"{name}: device entry"
    assert np.array_equal(got_host, want), f"{name}: host entry"


@pytest.mark.parametrize("per", list(EC.GEOMETRY))
def test_indexed_and_table_kernels_agree_over_the_device_table(det, per):
    """One board serves the three conventions: the table kernel over omr_indexed_weights_table_device's table
    gives the indexed case's digest."""
    import torch
    c = CASES[f"pay_indexed_per{per}"]
    rows = (c.first_ct + c.n_ct) * c.per_ct
    d_w = torch.zeros(rows * c.all, dtype=torch.int16, device="cuda:0")
    d_pv, d_pay, d_out = dev(c.pv), dev(c.payloads), out_buffer(c.n_ct)
    torch.cuda.synchronize()
    A.indexed_weights_table_device(c.seed, c.all, c.combos, c.first_ct + c.n_ct, c.per_ct, d_w.data_ptr())
    det.encode_payloads_device(d_pv.data_ptr(), d_pay.data_ptr(), c.D, c.offset, c.all,
                               d_w.data_ptr() + 2 * c.first_ct * c.per_ct * c.all, c.n_ct, c.per_ct, d_out.data_ptr())
    assert np.array_equal(host_of(d_out), c.expected)


# ---- the sums at the carry: omr_digest_merge and a session's updates --------------------------------------
S_ALL, S_D1 = 40, 33  # one index digit: 3 index and 3 payload ciphertexts; updates of 32 + 1 and of 7 messages


def tiled(x, n=3):
    return np.ascontiguousarray(np.broadcast_to(x, (n,) + x.shape))


@pytest.mark.parametrize("name", list(EC.merge_pairs()))
def test_merge_at_the_carry(det, name):
    a, b = EC.merge_pairs()[name]
    want = tiled(EC.add_mod(a, b))
    with det.digest_session(S_ALL, 0, EC.INDEX_SEED, EC.WEIGHT_SEED) as dg:
        assert (dg.info()["index_ct"], dg.info()["payload_ct"]) == (3, 3)
        dg.merge(tiled(a), tiled(b))  # 0 + a, 0 + b
        dg.merge(tiled(b), tiled(a))  # a + b, b + a
        idx, pay = dg.read()
        assert np.array_equal(idx, want) and np.array_equal(pay, want)
        # a word equal to q2 is refused and the digest stays as it is
        bad = tiled(a).copy()
        bad[2, 1, N2 - 1] = Q2
        for args in ((bad, None), (None, bad), (tiled(a), bad)):
            with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
                dg.merge(*args)
        idx, pay = dg.read()
        assert np.array_equal(idx, want) and np.array_equal(pay, want)


def test_session_updates_at_the_carry(det):
    mask = np.zeros(S_ALL, dtype=bool)
    mask[[3, 35]] = True
    ca, cb = PL.mixed_clues(mask, seed=8100)
    pay = np.random.default_rng(8101).integers(0, 256, (S_ALL, A.PAYLOAD_LENGTH)).astype(np.uint16)
    pv = det.detect_batch(ca, cb)
    assert int(pv.max()) < Q2
    i1, p1 = EC.board_digest(pv[:S_D1], pay[:S_D1], S_ALL, 0, EC.INDEX_SEED, EC.WEIGHT_SEED)
    i2, p2 = EC.board_digest(pv[S_D1:], pay[S_D1:], S_ALL, S_D1, EC.INDEX_SEED, EC.WEIGHT_SEED)
    (ai, wi), (ap, wp) = EC.steer(i2), EC.steer(p2)
    with det.digest_session(S_ALL, 0, EC.INDEX_SEED, EC.WEIGHT_SEED) as dg:
        dg.merge(ai, ap)
        dg.update(ca[S_D1:], cb[S_D1:], pay[S_D1:], S_D1)  # one workgroup: running digest + partial at the carry
        idx, pay_cts = dg.read()
        assert np.array_equal(idx, wi) and np.array_equal(pay_cts, wp)
        dg.update(ca[:S_D1], cb[:S_D1], pay[:S_D1], 0)     # two workgroups: 32 + 1
        idx, pay_cts = dg.read()
        now_i, now_p = EC.add_mod(wi, i1), EC.add_mod(wp, p1)
        assert np.array_equal(idx, now_i) and np.array_equal(pay_cts, now_p)
        (bi, wi2), (bp, wp2) = EC.steer(now_i), EC.steer(now_p)
        dg.merge(bi, bp)                                   # the merge onto a digest that updates built
        idx, pay_cts = dg.read()
        assert np.array_equal(idx, wi2) and np.array_equal(pay_cts, wp2)
    # the updates alone, in board order, are the model's digest of the board
    with det.digest_session(S_ALL, 0, EC.INDEX_SEED, EC.WEIGHT_SEED) as dg:
        dg.update(ca[:S_D1], cb[:S_D1], pay[:S_D1], 0)
        dg.update(ca[S_D1:], cb[S_D1:], pay[S_D1:], S_D1)
        idx, pay_cts = dg.read()
    assert np.array_equal(idx, EC.add_mod(i1, i2)) and np.array_equal(pay_cts, EC.add_mod(p1, p2))
    assert idx.any() and pay_cts.any()


# ---- omr_encode_indices_device's argument check -----------------------------------------------------------
def test_index_entry_refuses_before_enqueuing(det):
    import torch
    D = 5
    d_pv, d_out = dev(EC.random_pv("args", D)), out_buffer(2)
    U = EC.U64
    bad = [
        dict(off=U - 1, all=U),             # offset + D wraps past 2^64 to 3 <= all
        dict(off=U, D=2, all=U),            # offset = all, D > 0: wraps to 1
        dict(off=8, all=12),                # plainly beyond the board
        dict(n_ct=65536),                   # the grid's y extent
        dict(n_ct=0),
        dict(pv=0),                         # NULL pv with D > 0
    ]
    for kw in bad:
        a = dict(pv=d_pv.data_ptr(), D=D, off=0, all=100, n_ct=2)
        a.update(kw)
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            det.encode_indices_device(a["pv"], a["D"], a["off"], a["all"], EC.INDEX_SEED, 0, a["n_ct"],
                                      d_out.data_ptr())
    assert (host_of(d_out) == np.uint64(2**64 - 1)).all()  # nothing was written
    # the host entry inherits the range check
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        det.encode_pertinent_indices(A.RetrievalParams(U, 0), EC.random_pv("args", D), EC.INDEX_SEED, 0, U - 1)
    # and the entry still works: the last messages of the largest board
    det.encode_indices_device(d_pv.data_ptr(), D, U - D, U, EC.INDEX_SEED, 0, 2, d_out.data_ptr())
    assert int(host_of(d_out).max()) < Q2
